"""Inputs, the oracle's results and a restatement of the kernel's algorithm for batched NMS (csrc/nms.hip).  NumPy and oracle/ only:
tests/test_nms_cases_cpu.py checks the cases themselves on a machine without a GPU, tests/test_nms_gpu.py launches the kernel on them.

The reference is oracle.yolo2_ref.non_max_suppress_fast per image (pinned to the reference's own goldens in tests/test_oracle.py); every
comparison is exact, bit for bit.  `paths(name)` says, from the inputs alone, which of the kernel's code paths a case takes (full or partial
sort, the number of 64-candidate groups, suppression across groups, the depth of the tie-breaks, the LDS request), so that the CPU test can
assert that the table as a whole reaches every path.  `model(name, mutation)` restates the KERNEL's algorithm (lexicographic key on the
original scores, K from the threshold, a `removed` flag per sorted position, zeroing at the end) with switches for the ways it could be
subtly wrong: without a switch it must equal the oracle on every case, with one it must differ on some.

Inputs are finite f32 with xy_min <= xy_max and no NaN anywhere: the reference asserts on, or leaves undefined, anything else.  Every case
and every result is built once and cached; the arrays are read-only."""
import functools

import numpy as np

from oracle import yolo2_ref as R

TIE = np.float32(0.25)        # the repeated score of the `uniform` recipes
GROUP = 64                    # csrc/nms.hip Y2_NMS_GROUP: candidates per overlap-row group, and boxes per 64-bit word
LDS_DEFAULT = 64 * 1024       # above this yolo2_nms raises hipFuncAttributeMaxDynamicSharedMemorySize
N_LIMIT = 4096                # include/yolo2_hip.h

# name -> (B, N, C, threshold, threshold_iou, recipe, seed, with_order)
CASES = {}

# ---- sizes: 1 / 2 (empty scan, one pair); 63..129 (one or two 64-box words, one or two candidate groups); 255..257 (boxes per thread 1 -> 2);
# 511 / 513 / 1025 (NP doubles); 2010 / 2011 (the LDS request crosses 64 KiB); 4095 / 4096 (the documented limit)
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1025, 2010, 2011, 4095, 4096)
for _i, _n in enumerate(SIZES):
    CASES['n%d' % _n] = (2, _n, 3, 0.1, 0.4, 'uniform', 100 + _i, True)

# ---- candidate counts: exactly K scores of class 0 above the threshold (partial sort, np = pow2 >= K); class 1 is the last one (full sort)
COUNTS = (0, 1, 2, 63, 64, 65, 128, 129, 256, 257, 299, 300)
for _i, _k in enumerate(COUNTS):
    CASES['k%d' % _k] = (2, 300, 2, 0.3, 0.4, 'planted:%d' % _k, 200 + _i, True)

CASES.update({
    # ---- thresholds
    'thr_neg1': (2, 200, 3, -1.0, 0.4, 'uniform', 301, True),            # every box a candidate; a suppressed box (score 0 > -1) still suppresses
    'thr_neg1_n4096': (1, 4096, 1, -1.0, 0.4, 'uniform', 310, True),      # K = N at the limit: 64 groups of 64 rows, every one OR-ed in
    'thr_negzero': (2, 200, 3, -0.0, 0.4, 'zeros', 302, True),           # -0.0 is not negative: behaves as 0.0
    'thr_zero': (2, 200, 3, 0.0, 0.4, 'zeros', 303, True),               # ~30 % of the scores are +0.0 or -0.0: never candidates
    'eval_regime': (2, 845, 20, 0.005, 0.45, 'eval', 304, True),         # eval.py -t 0.005 --threshold_iou 0.45
    'thr_equals_score': (2, 200, 3, float(TIE), 0.4, 'uniform', 305, True),      # 15 % of the scores equal the threshold: `<=` skips them
    'thr_one': (2, 200, 3, 1.0, 0.4, 'ones', 306, True),                 # nothing is a candidate, 15 % of the scores are exactly 1.0
    'iou_zero': (2, 200, 3, 0.3, 0.0, 'uniform', 307, True),             # every later box goes, disjoint ones included (0 >= 0)
    'iou_one_dups': (2, 200, 3, 0.3, 1.0, 'dups5', 308, True),           # 40 boxes five times each: IoU exactly 1
    'iou_above_one': (2, 200, 3, 0.3, 1.5, 'dups5', 309, True),          # nothing goes
    # ---- interface
    'no_order': (2, 300, 3, 0.1, 0.4, 'uniform', 401, False),            # order_out = NULL: no class is fully sorted
    'c1': (2, 300, 1, 0.1, 0.4, 'uniform', 402, True),                   # the only class is the last one
    'c1_no_order': (2, 300, 1, 0.1, 0.4, 'uniform', 402, False),
    'c80_b3': (3, 845, 80, 0.3, 0.4, 'sparse', 403, True),
    'side_stream': (2, 300, 3, 0.1, 0.4, 'uniform', 404, True),          # launched on a non-default stream by the GPU test
    # ---- ties
    'tie_through_suppressed': (2, 96, 3, 0.3, 0.4, 'tie_through_suppressed', 501, True),
    'tie_chain3': (2, 120, 5, 0.3, 0.4, 'tie_chain3', 502, True),        # ties of class 4 broken only by class 1
    'tie_index': (2, 120, 3, 0.3, 0.4, 'tie_index', 503, True),          # whole rows equal: broken only by the box index
    # ---- geometry
    'zero_area': (2, 160, 3, 0.3, 0.4, 'zero_area', 601, True),
    'zero_area_iou_zero': (2, 160, 3, 0.3, 0.0, 'zero_area', 602, True),
    'at_threshold_straddle': (2, 130, 1, 0.3, None, 'at_threshold', 603, True),   # thr_iou = the IoU of the pair at sorted positions 63 / 64
    'at_threshold_straddle_no_order': (2, 130, 1, 0.3, None, 'at_threshold', 603, False),      # the same through the partial sort
})
SIDE_STREAM_CASE = 'side_stream'
NAMES = tuple(CASES)


def pow2_at_least(n, floor=1):
    p = floor
    while p < n:
        p <<= 1
    return p


def lds_bytes(N):
    """The dynamic LDS request of yolo2_nms (csrc/nms.hip, `const size_t lds = ...` in yolo2_nms): skey, sidx, key (3 N floats), up to 16 bytes
    of alignment, sbox (N float4), perm (NP ints, NP = pow2 >= N, at least 2) and cnt (256 ints).  If that line changes, this one must, and the
    2010 / 2011 pair of SIZES moves to the new 64 KiB boundary (tests/test_nms_cases_cpu.py asserts that the pair straddles it)."""
    NP = pow2_at_least(N, 2)
    return 4 * 3 * N + 16 + 4 * 4 * N + 4 * (NP + 256)


# ---------------------------------------------------------------------------------------------------------------------
# recipes
# ---------------------------------------------------------------------------------------------------------------------

def _boxes(rng, B, N, extent=None):
    """Centres uniform in a square, sides 0.5 .. 5.5 (tests/test_kernels_gpu.py's boxes); the square grows with N from 4 to 13 so that small
    cases still have overlapping boxes."""
    extent = float(np.clip(13.0 * np.sqrt(N / 845.0), 4.0, 13.0)) if extent is None else extent
    cen = rng.uniform(0, extent, (B, N, 2)).astype(np.float32)
    wh = rng.uniform(0.5, 5.5, (B, N, 2)).astype(np.float32)
    return (cen - wh / 2).astype(np.float32), (cen + wh / 2).astype(np.float32)


def _uniform_scores(rng, B, N, C, tie=TIE):
    conf = rng.uniform(0, 0.5, (B, N, C)).astype(np.float32)
    conf[rng.rand(B, N, C) < 0.15] = tie
    return conf


def _recipe_uniform(rng, B, N, C, thr):
    return (_uniform_scores(rng, B, N, C),) + _boxes(rng, B, N)


def _recipe_ones(rng, B, N, C, thr):
    return (_uniform_scores(rng, B, N, C, np.float32(1.0)),) + _boxes(rng, B, N)


def _recipe_zeros(rng, B, N, C, thr):
    conf = _uniform_scores(rng, B, N, C)
    z = rng.rand(B, N, C)
    conf[z < 0.15] = np.float32(0.0)
    conf[(z >= 0.15) & (z < 0.30)] = np.float32(-0.0)
    return (conf,) + _boxes(rng, B, N)


def _recipe_planted(rng, B, N, C, thr, K):
    """Exactly K scores of class 0 above the threshold (a tenth of them tied), the others at or below it; the other classes uniform.  The
    lowest candidate has the box of the highest one, so with K > 64 a candidate of a later group is certainly suppressed from group 0."""
    conf = _uniform_scores(rng, B, N, C)
    mn, mx = _boxes(rng, B, N, 6.0)
    for b in range(B):
        col = rng.uniform(0, thr - 0.01, N).astype(np.float32)
        col[rng.rand(N) < 0.05] = np.float32(thr)             # at the threshold: not a candidate
        hot = rng.choice(N, K, replace=False)
        col[hot] = rng.uniform(thr + 0.01, 0.95, K).astype(np.float32)
        col[hot[rng.rand(K) < 0.1]] = np.float32(0.5)
        if K >= 2:
            col[hot[0]], col[hot[1]] = np.float32(0.97), np.float32(thr + 0.005)
            mn[b, hot[1]], mx[b, hot[1]] = mn[b, hot[0]], mx[b, hot[0]]
        conf[b, :, 0] = col
    return conf, mn, mx


def _recipe_sparse(rng, B, N, C, thr):
    """tests/test_kernels_gpu.py's sparse detections: 40 hot scores per image over a floor below the threshold."""
    conf = rng.uniform(0, 0.05, (B, N, C)).astype(np.float32)
    for b in range(B):
        hot = rng.choice(N, 40, replace=False)
        conf[b, hot, rng.randint(0, C, 40)] = rng.uniform(0.3, 0.95, 40).astype(np.float32)
    return (conf,) + _boxes(rng, B, N)


def _recipe_eval(rng, B, N, C, thr):
    """Scores skewed as a detector's are (0.9 u^8: the median is 0.0035, 95 % are below 0.6), with 2 % at the threshold and 40 confident ones
    per image.  About 47 % of the scores are above 0.005, so a class has some 400 candidates of 845: denser than a trained network gives
    (a harder case), but every class takes the partial sort with several candidate groups, which a handful of candidates would not."""
    conf = (rng.uniform(0, 1, (B, N, C)) ** 8 * 0.9).astype(np.float32)
    conf[rng.rand(B, N, C) < 0.02] = np.float32(0.005)        # at the threshold
    for b in range(B):
        hot = rng.choice(N, 40, replace=False)
        conf[b, hot, rng.randint(0, C, 40)] = rng.uniform(0.3, 0.95, 40).astype(np.float32)
    return (conf,) + _boxes(rng, B, N)


def _recipe_dups5(rng, B, N, C, thr):
    assert N % 5 == 0
    mn, mx = _boxes(rng, B, N // 5, 13.0)
    pick = np.stack([rng.permutation(np.repeat(np.arange(N // 5), 5)) for _ in range(B)])
    mn = np.stack([mn[b, pick[b]] for b in range(B)])
    mx = np.stack([mx[b, pick[b]] for b in range(B)])
    return _uniform_scores(rng, B, N, C), mn, mx


def _recipe_tie_through_suppressed(rng, B, N, C, thr):
    """N / 3 copies of a three-box motif, far apart.  X = box 3m, Y = 3m+1, Z = 3m+2: IoU(X, Y) = 0.6, IoU(Y, Z) = 0.43, IoU(X, Z) = 0.21.
    In class c-1: Z 0.9 > Y 0.8 > X 0.5, so Z suppresses Y there (its score becomes 0 < X's 0.5).  In class c: X and Y tie at 0.7, Z is 0.
    On the ORIGINAL scores Y sorts before X and suppresses it; on the mutated column X would come first.  Image 0 has (c-1, c) = (0, 1) and
    a random last class, image 1 has (1, 2) with a constant class 0, so there the tied class is the one whose order is reported."""
    assert N % 3 == 0 and C == 3
    M = N // 3
    motif_mn = np.float32([[0, 0], [0.5, 0], [1.3, 0]])
    motif_mx = motif_mn + np.float32(2)
    off = np.stack([np.float32(10) * (np.arange(M) % 8), np.float32(10) * (np.arange(M) // 8)], 1).astype(np.float32)
    mn = np.tile((off[:, None, :] + motif_mn[None]).reshape(1, N, 2), (B, 1, 1)).astype(np.float32)
    mx = np.tile((off[:, None, :] + motif_mx[None]).reshape(1, N, 2), (B, 1, 1)).astype(np.float32)
    conf = np.zeros((B, N, C), np.float32)
    for b in range(B):
        lo = b % 2                                               # the class c-1
        conf[b, :, lo] = np.tile(np.float32([0.5, 0.8, 0.9]), M)
        conf[b, :, lo + 1] = np.tile(np.float32([0.7, 0.7, 0.0]), M)
        if lo == 0:
            conf[b, :, 2] = rng.uniform(0, 0.5, N).astype(np.float32)
        else:
            conf[b, :, 0] = np.float32(0.6)
    return conf, mn, mx


def _recipe_tie_chain3(rng, B, N, C, thr):
    """Classes 2, 3, 4 hold one of two values per box, the same in all three for most boxes; class 1 is distinct everywhere: a tie of
    class 4 walks classes 3 and 2 and ends at class 1."""
    assert C == 5
    conf = rng.uniform(0.05, 0.95, (B, N, C)).astype(np.float32)
    level = rng.choice(np.float32([0.35, 0.6]), (B, N, 1))
    conf[:, :, 2:] = level
    flip = rng.rand(B, N) < 0.2
    conf[:, :, 3][flip] = np.float32(0.45)                       # some ties end one class back
    return (conf,) + _boxes(rng, B, N, 6.0)


def _recipe_tie_index(rng, B, N, C, thr):
    conf = rng.choice(np.float32([0.1, 0.35, 0.6]), (B, N, C)).astype(np.float32)
    return (conf,) + _boxes(rng, B, N, 6.0)


def _recipe_zero_area(rng, B, N, C, thr):
    """A quarter each: zero width, zero height, zero area at one of four shared points (identical boxes), ordinary."""
    mn, mx = _boxes(rng, B, N, 5.0)
    kind = np.arange(N) % 4
    mx[:, kind == 0, 0] = mn[:, kind == 0, 0]
    mx[:, kind == 1, 1] = mn[:, kind == 1, 1]
    points = rng.uniform(1, 4, (B, 4, 2)).astype(np.float32)
    at = points[:, rng.randint(0, 4, (kind == 2).sum())]
    mn[:, kind == 2] = at
    mx[:, kind == 2] = at
    return _uniform_scores(rng, B, N, C, np.float32(0.4)), mn, mx


def _iou_f32(mn1, mx1, mn2, mx2, contracted=False):
    a1 = (mx1[0] - mn1[0]) * (mx1[1] - mn1[1])
    a2 = (mx2[0] - mn2[0]) * (mx2[1] - mn2[1])
    w = np.maximum(np.minimum(mx1[0], mx2[0]) - np.maximum(mn1[0], mn2[0]), np.float32(0))
    h = np.maximum(np.minimum(mx1[1], mx2[1]) - np.maximum(mn1[1], mn2[1]), np.float32(0))
    inter = w * h
    union = a1 + (a2 - inter) if contracted else (a1 + a2) - inter
    return inter / np.maximum(union, np.float32(1e-10))


def _recipe_at_threshold(rng, B, N, C, thr):
    """The reference golden's `at_threshold` construction (a pair whose IoU IS the IoU threshold, so `>=` must fire) at sorted positions 63
    and 64: the suppressor is the last candidate of group 0 and the bit it sets is the first one of the second 64-box word.  All other boxes are
    disjoint from everything.  The pair is drawn until (a1 + a2) - inter and a1 + (a2 - inter) round to different unions with the reference's
    IoU the larger one, so that the other association misses the threshold."""
    assert C == 1 and N > 66
    while True:
        amn = rng.uniform(0, 1, 2).astype(np.float32)
        amx = (amn + rng.uniform(1, 3, 2)).astype(np.float32)
        bmn = (amn + rng.uniform(0.1, 0.9, 2)).astype(np.float32)
        bmx = (bmn + rng.uniform(1, 3, 2)).astype(np.float32)
        v, w = _iou_f32(amn, amx, bmn, bmx), _iou_f32(amn, amx, bmn, bmx, True)
        if v > w and v == R.iou(amn, amx, bmn, bmx):
            break
    mn = np.zeros((B, N, 2), np.float32)
    mx = np.zeros((B, N, 2), np.float32)
    conf = np.zeros((B, N, 1), np.float32)
    for b in range(B):
        where = rng.permutation(N)                               # sorted position -> box index
        score = np.linspace(0.95, 0.35, N).astype(np.float32)    # distinct, descending, all above the threshold
        conf[b, where, 0] = score
        cell = 10 + 10 * np.arange(N)
        mn[b, where] = np.stack([cell, cell], 1).astype(np.float32)
        mx[b, where] = mn[b, where] + np.float32(1)
        mn[b, where[63]], mx[b, where[63]] = amn, amx
        mn[b, where[64]], mx[b, where[64]] = bmn, bmx
    return conf, mn, mx, float(v)


RECIPES = {'uniform': _recipe_uniform, 'ones': _recipe_ones, 'zeros': _recipe_zeros, 'sparse': _recipe_sparse, 'eval': _recipe_eval,
           'dups5': _recipe_dups5, 'tie_through_suppressed': _recipe_tie_through_suppressed, 'tie_chain3': _recipe_tie_chain3,
           'tie_index': _recipe_tie_index, 'zero_area': _recipe_zero_area, 'at_threshold': _recipe_at_threshold}


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case(name):
    """{'name', 'B', 'N', 'C', 'thr', 'thr_iou', 'with_order', 'conf' [B,N,C], 'xy_min' [B,N,2], 'xy_max' [B,N,2]}: f32, read-only."""
    B, N, C, thr, thr_iou, recipe, seed, with_order = CASES[name]
    rng = np.random.RandomState(seed)
    kind, _, arg = recipe.partition(':')
    out = _recipe_planted(rng, B, N, C, thr, int(arg)) if kind == 'planted' else RECIPES[kind](rng, B, N, C, thr)
    if thr_iou is None:
        thr_iou = out[3]
    conf, mn, mx = out[:3]
    assert conf.shape == (B, N, C) and mn.shape == mx.shape == (B, N, 2)
    assert conf.dtype == mn.dtype == mx.dtype == np.float32
    assert np.all(np.isfinite(conf)) and np.all(np.isfinite(mn)) and np.all(np.isfinite(mx)) and np.all(mn <= mx)
    # the kernel takes the thresholds as floats: what it compares with is the f32 value
    return {'name': name, 'B': B, 'N': N, 'C': C, 'thr': float(np.float32(thr)), 'thr_iou': float(np.float32(thr_iou)), 'with_order': with_order,
            'conf': _frozen(conf), 'xy_min': _frozen(mn), 'xy_max': _frozen(mx)}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle per image: (conf_out [B,N,C] f32, order [B,N] int64), read-only."""
    c = case(name)
    conf = c['conf'].copy()
    order = np.stack([R.non_max_suppress_fast(conf[b].reshape(c['N'], 1, c['C']), c['xy_min'][b], c['xy_max'][b], c['thr'], c['thr_iou'])
                      for b in range(c['B'])])
    return _frozen(conf), _frozen(order)


def bits(a):
    """f32 array -> its bit patterns: zeros keep their sign under this comparison."""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's algorithm, restated
# ---------------------------------------------------------------------------------------------------------------------

MUTATIONS = ('index_ties', 'ties_read_mutated', 'dead_suppresses', 'neg_thr_dead_stops', 'lt_thr', 'gt_iou', 'candidates_only', 'group_local',
             'contracted_union')


def _sorted_positions(cols, c, idx):
    """`idx` (box indices, ascending) in the kernel's order for class c: column c descending, then c-1 .. 0 descending, then box index
    ascending (csrc/nms.hip sorts_before).  np.lexsort: the LAST key is the primary one; -0.0 and 0.0 compare equal, as in the kernel."""
    keys = [idx] + [-cols[idx, cc] for cc in range(c + 1)]
    return idx[np.lexsort(keys)]


def _tie_walk(cols, c, seq):
    """Over neighbours in the sorted sequence whose class-c scores tie: (the largest number of earlier classes read to separate them, the
    number of pairs that only the box index separates)."""
    if len(seq) < 2:
        return 0, 0
    a, b = seq[:-1], seq[1:]
    tied = cols[a, c] == cols[b, c]
    read = np.zeros(len(a), np.int64)
    for cc in range(c - 1, -1, -1):
        read[tied] += 1
        tied = tied & (cols[a, cc] == cols[b, cc])
    return int(read.max()), int(tied.sum())


def _model_image(conf, mn, mx, thr, thr_iou, with_order, mutation):
    """One image.  conf [N, C] is updated in place; returns (order of the last class, per-class path statistics)."""
    N, C = conf.shape
    thr, thr_iou = np.float32(thr), np.float32(thr_iou)
    conf0 = conf.copy()                                          # the snapshot yolo2_nms takes into `ws`
    wh = mx - mn
    area = wh[:, 0] * wh[:, 1]
    everything = np.arange(N)
    order, stats = None, []
    negative = not (np.float32(0) <= thr)
    for c in range(C):
        # classes are independent in the kernel (one workgroup each, all reading the snapshot); only the `ties_read_mutated` switch makes
        # their order matter, and then it is the reference's: one class after the other
        cols = conf0.copy() if mutation != 'ties_read_mutated' else np.concatenate([conf[:, :c], conf0[:, c:]], 1)
        if mutation == 'index_ties':
            cols = np.concatenate([np.zeros((N, c), np.float32), conf0[:, c:]], 1)
        key = conf0[:, c]
        cand = key >= thr if mutation == 'lt_thr' else key > thr
        full = negative or (with_order and c == C - 1)
        if full:
            sidx = _sorted_positions(cols, c, everything)
            K = N if negative else int(cand.sum())
            walked = sidx
        else:
            K = int(cand.sum())
            sidx = np.concatenate([_sorted_positions(cols, c, everything[cand]), everything[~cand]])     # the others unsorted, behind
            walked = sidx[:K]
        if c == C - 1:
            order = sidx.copy() if full else None
        skey = key[sidx]
        smn, smx, sarea = mn[sidx], mx[sidx], area[sidx]
        removed = np.zeros(N, bool)                              # per sorted position: the kernel's `removed` words
        seen = np.zeros(N, bool)                                 # what the walk of the current group can see of them
        cross = alive = 0
        for p in range(min(K, N - 1)):
            if mutation == 'group_local' and p % GROUP == 0:
                seen = np.zeros(N, bool)
            dead = seen[p]
            if negative:
                if dead and mutation == 'neg_thr_dead_stops':
                    continue
                cur = np.float32(0) if dead else skey[p]
            else:
                cur = skey[p] if mutation == 'dead_suppresses' else (np.float32(0) if dead else skey[p])
            if (cur < thr) if mutation == 'lt_thr' else (cur <= thr):
                continue
            alive += 1
            lo = np.maximum(smn[p], smn[p + 1:])
            hi = np.minimum(smx[p], smx[p + 1:])
            d = np.maximum(hi - lo, np.float32(0))
            inter = d[:, 0] * d[:, 1]
            union = sarea[p] + (sarea[p + 1:] - inter) if mutation == 'contracted_union' else (sarea[p] + sarea[p + 1:]) - inter
            iou = inter / np.maximum(union, np.float32(1e-10))
            hit = iou > thr_iou if mutation == 'gt_iou' else iou >= thr_iou
            if mutation == 'candidates_only':
                hit[max(K - (p + 1), 0):] = False
            q = p + 1 + np.flatnonzero(hit)
            new = q[~removed[q]]
            cross += int(((new >= GROUP) & (new < K) & (new // GROUP > p // GROUP)).sum())
            removed[q] = True
            seen[q] = True
        conf[sidx[removed], c] = np.float32(0)                   # zeroed at the end, as the kernel does
        depth, by_index = _tie_walk(conf0, c, walked)
        np_sort = pow2_at_least(N, 2) if full else pow2_at_least(K)
        stats.append({'c': c, 'K': K, 'full': bool(full), 'np': np_sort, 'NP': pow2_at_least(N, 2), 'groups': -(-K // GROUP), 'chunks': -(-N // GROUP),
                      'per': -(-N // 256), 'cross_group': cross, 'alive': alive, 'removed': int(removed.sum()), 'tie_depth': depth,
                      'index_ties': by_index, 'lds_bytes': lds_bytes(N)})
    return order, stats


@functools.lru_cache(maxsize=None)
def _model(name, mutation):
    c = case(name)
    conf = c['conf'].copy()
    orders, stats = [], []
    for b in range(c['B']):
        order, st = _model_image(conf[b], c['xy_min'][b], c['xy_max'][b], c['thr'], c['thr_iou'], c['with_order'], mutation)
        orders.append(order)
        stats += [dict(s, b=b) for s in st]
    order = None if orders[0] is None else _frozen(np.stack(orders).astype(np.int64))
    return _frozen(conf), order, tuple(stats)


def model(name, mutation=None):
    """The kernel's algorithm on a case: (conf_out [B,N,C], order [B,N] or None where no full order exists).  `mutation` is None or one
    of MUTATIONS."""
    assert mutation is None or mutation in MUTATIONS
    conf, order, _ = _model(name, mutation)
    return conf, order


def paths(name):
    """What the kernel does on this case, one dict per (image b, class c): K (candidates), full (full or partial sort), np (the length the
    bitonic network runs over), NP, groups = ceil(K / 64), chunks = ceil(N / 64), per (boxes per thread of the candidate count), cross_group
    (candidates at sorted position >= 64 first suppressed by a candidate of an earlier group), alive (candidates that suppress), removed,
    tie_depth (the most earlier classes a tie-break between neighbours in the sorted sequence reads), index_ties (neighbours only the box
    index separates), lds_bytes."""
    return _model(name, None)[2]
