"""Inputs for yolo2_wbf and yolo2_tta_gather (csrc/tta.hip), in the manner of tests/soft_nms_cases.py: a named table of hand-made and seeded
cases, built once, cached, read-only.  NumPy only: tests/test_tta_cpu.py checks the table on a machine without a GPU, tests/test_tta_gpu.py
launches the kernels on it.  The expected results are tests/tta_ref.py's (the specification); `model(name, variant)` restates the fusion box
by box with switches for the ways an implementation could be subtly wrong.

Scores are finite except in `nan_negative`; boxes are finite with xy_min <= xy_max."""
import functools

import numpy as np

import tta_ref as T
from nms_cases import _boxes, _frozen, bits  # noqa: F401  (bits: for the tests)

F = np.float32


def _one(scores, boxes):
    """One image, one class: conf [1,M,1], xy_min, xy_max [1,M,2]."""
    b = np.asarray(boxes, F).reshape(1, -1, 4)
    return np.asarray(scores, F).reshape(1, -1, 1), b[:, :, :2].copy(), b[:, :, 2:].copy()


# ---------------------------------------------------------------------------------------------------------------------
# hand-made cases: name -> (conf, xy_min, xy_max, threshold, fuse_iou, V, max_per_class, R)
# ---------------------------------------------------------------------------------------------------------------------

def search_singleton(seed, draws):
    """At most `draws` seeded (s, x) with s in (0.05, 1) and x in (1, 13): the first for which (s * x) / s is not x in f32."""
    rng = np.random.RandomState(seed)
    for n in range(draws):
        s, x = F(rng.uniform(0.05, 1)), F(rng.uniform(1, 13))
        if (s * x) / s != x:
            return n, s, x
    return None


SINGLETON_SEARCH = dict(seed=0, draws=200)


def _hand():
    h = {}
    # IoU of the two is 16 / 32 = 0.5 = fuse_iou: they join (>=); the fused box is (0, 0, 4, (3 + 2) / 1) with score (1 / 2) * 2 / 2
    h['hand2'] = _one([0.75, 0.25], [[0, 0, 4, 4], [0, 0, 4, 8]]) + (0.1, 0.5, 2, 8, 4)
    # a third box equal to the fused one joins: sums (0, 0, 4.5, 5.625) / 1.125, score (1.125 / 3) * 2 / 2
    h['hand3'] = _one([0.75, 0.25, 0.125], [[0, 0, 4, 4], [0, 0, 4, 8], [0, 0, 4, 5]]) + (0.1, 0.5, 2, 8, 4)
    # the third box overlaps the fused box (0, 0, 4, 5) by 14 / 24 and the leader (0, 0, 4, 4) by 10 / 24
    h['fused_not_leader'] = _one([0.75, 0.25, 0.125], [[0, 0, 4, 4], [0, 0, 4, 8], [0, 1.5, 4, 6]]) + (0.1, 0.5, 2, 8, 4)
    # equal scores, disjoint boxes: the lower pooled index opens the first cluster
    h['score_tie'] = _one([0.5, 0.5], [[0, 0, 2, 2], [4, 0, 6, 2]]) + (0.1, 0.5, 2, 8, 4)
    # the third box overlaps both clusters by 2 / 10 exactly, and fuse_iou is that value: the lower cluster takes it
    h['iou_tie'] = _one([0.75, 0.5, 0.25], [[0, 0, 2, 2], [4, 0, 6, 2], [1, 0, 5, 2]]) + (0.1, float(F(2) / F(10)), 2, 8, 4)
    # T = 3 > V = 2 (identical boxes), and T = 1 < V = 2
    h['t_above_v'] = _one([0.75, 0.5, 0.25], [[0, 0, 4, 4]] * 3) + (0.1, 0.5, 2, 8, 4)
    h['t_below_v'] = _one([0.75], [[0, 0, 4, 4]]) + (0.1, 0.5, 2, 8, 4)
    found = search_singleton(**SINGLETON_SEARCH)
    assert found is not None
    _, s, x = found
    h['singleton_exact'] = _one([s], [[0, 0, x, x]]) + (0.01, 0.5, 1, 8, 4)
    # eight disjoint boxes: exactly max_per_class clusters / one more; exactly R rows / one more
    grid = [[3 * i, 0, 3 * i + 2, 2] for i in range(8)]
    sc = np.linspace(0.9, 0.2, 8)
    h['clusters_fit'] = _one(sc, grid) + (0.1, 0.5, 2, 8, 8)
    h['clusters_over'] = _one(sc, grid) + (0.1, 0.5, 2, 7, 8)
    h['rows_fit'] = _one(sc, grid) + (0.1, 0.5, 2, 8, 8)
    h['rows_over'] = _one(sc, grid) + (0.1, 0.5, 2, 8, 7)
    return h


# ---------------------------------------------------------------------------------------------------------------------
# seeded cases: name -> (B, M, C, threshold, fuse_iou, V, max_per_class, R or None (= M * C: every box in every class), recipe, seed)
# ---------------------------------------------------------------------------------------------------------------------
# 63 / 64 / 65: one or two 64-box chunks in the compaction, and the sort network's size; 257: two chunks in one wave, thread 0 owns two
# clusters when every box opens one; 1024: four chunks per wave
SEEDED = {}
for _i, _m in enumerate((1, 63, 64, 65, 257, 1024)):
    SEEDED['m%d' % _m] = (1 if _m > 300 else 2, _m, 2, 0.05, 0.55, 2, 1024, None, 'overlap', 2100 + _i)
SEEDED.update({
    'c1_b1_v1': (1, 200, 1, 0.05, 0.55, 1, 256, None, 'groups', 2201),
    'c3_b3_v2': (3, 200, 3, 0.05, 0.55, 2, 256, None, 'groups', 2202),
    'c20_b1_v5': (1, 128, 20, 0.05, 0.55, 5, 256, None, 'groups', 2203),
    'c80_b3_v5': (3, 65, 80, 0.05, 0.55, 5, 256, None, 'groups', 2204),
    'dense': (2, 512, 2, 0.05, 0.55, 5, 64, None, 'groups', 2301),                  # sixteen boxes per group: many joins per cluster
    'disjoint': (2, 300, 2, 0.05, 0.55, 2, 1024, None, 'disjoint', 2302),           # every candidate opens a cluster: 300 > 256, two per thread
    'equal_scores': (2, 160, 3, 0.05, 0.55, 2, 256, None, 'tie_scores', 2303),      # three score levels: the pooled index decides
    'zero_area': (2, 160, 2, 0.05, 0.55, 2, 256, None, 'zero_area', 2304),          # the 1e-10 floor
    'thr_zero': (2, 200, 3, 0.0, 0.55, 2, 256, None, 'zeros', 2305),                # +0.0 and -0.0 are no candidates
    'nan_negative': (2, 200, 3, 0.0, 0.55, 2, 256, None, 'nan_negative', 2306),     # nor are NaN and negative scores
    'empty_class': (2, 128, 3, 0.05, 0.55, 2, 256, None, 'empty_class', 2307),      # class 1 has no candidate, classes 0 and 2 have
    'subnormal': (1, 128, 2, 0.0, 0.55, 2, 256, None, 'subnormal', 2308),           # scores, sums and products in the f32 subnormal range
    'iou_zero': (1, 100, 2, 0.05, 0.0, 2, 256, None, 'overlap', 2309),              # every overlap, 0 included, is >= fuse_iou: one cluster
    'iou_above_one': (1, 100, 2, 0.05, 1.5, 2, 256, None, 'groups', 2310),          # nothing joins
    'max_candidates': (1, T.MAX_CANDIDATES, 1, 0.0, 0.55, 5, 1024, None, 'groups', 2401),          # the longest chain the library takes
    'max_candidates_plus1': (1, T.MAX_CANDIDATES + 1, 2, 0.0, 0.55, 5, 1024, None, 'overflow_class0', 2402),      # bit 0; class 1 still emits
    'row_overflow_b3': (3, 64, 3, 0.05, 0.55, 2, 256, 20, 'disjoint', 2403),        # bit 2 with several classes and images
    # the emit kernel scans 256 classes at a time: candidates in classes 0, 3, 254, 255 (first pass) and 256, 258, 511, 512, 513 (the second
    # and third pass, with the rows of the earlier passes carried over)
    'c514_b2': (2, 48, 514, 0.05, 0.55, 2, 64, 400, 'classes_around_256', 2404),
})
CLASSES_AROUND_256 = (0, 3, 254, 255, 256, 258, 511, 512, 513)


def _scores(rng, B, M, C, lo=0.06, hi=0.95):
    return rng.uniform(lo, hi, (B, M, C)).astype(F)


def _groups(rng, B, M, per=16):
    """ceil(M / per) group boxes 10 apart, each pooled box a jittered copy of one: the views' detections of one object."""
    G = -(-M // per)
    cen = np.stack([10.0 * (np.arange(G) % 16), 10.0 * (np.arange(G) // 16)], 1).astype(F)
    pick = np.stack([rng.permutation(np.repeat(np.arange(G), per))[:M] for _ in range(B)])
    c = cen[pick] + rng.uniform(-0.2, 0.2, (B, M, 2)).astype(F)
    wh = rng.uniform(3.5, 4.5, (B, M, 2)).astype(F)
    return (c - wh / 2).astype(F), (c + wh / 2).astype(F)


def _recipe_overlap(rng, B, M, C):
    return (_scores(rng, B, M, C),) + _boxes(rng, B, M)


def _recipe_groups(rng, B, M, C):
    return (_scores(rng, B, M, C),) + _groups(rng, B, M)


def _recipe_disjoint(rng, B, M, C):
    cell = np.stack([3 * (np.arange(M) % 32), 3 * (np.arange(M) // 32)], 1).astype(F)
    mn = np.stack([cell[rng.permutation(M)] for _ in range(B)])
    return _scores(rng, B, M, C), mn, mn + F(2)


def _recipe_tie_scores(rng, B, M, C):
    return (rng.choice(F([0.1, 0.35, 0.6]), (B, M, C)).astype(F),) + _groups(rng, B, M, 8)


def _recipe_zero_area(rng, B, M, C):
    """A quarter each: zero width, zero height, zero area at one of four shared points (identical boxes), ordinary."""
    mn, mx = _boxes(rng, B, M, 5.0)
    kind = np.arange(M) % 4
    mx[:, kind == 0, 0] = mn[:, kind == 0, 0]
    mx[:, kind == 1, 1] = mn[:, kind == 1, 1]
    points = rng.uniform(1, 4, (B, 4, 2)).astype(F)
    at = points[:, rng.randint(0, 4, (kind == 2).sum())]
    mn[:, kind == 2] = at
    mx[:, kind == 2] = at
    return _scores(rng, B, M, C), mn, mx


def _recipe_zeros(rng, B, M, C):
    conf = _scores(rng, B, M, C, 0.0, 0.9)
    z = rng.rand(B, M, C)
    conf[z < 0.15] = F(0.0)
    conf[(z >= 0.15) & (z < 0.30)] = F(-0.0)
    return (conf,) + _groups(rng, B, M)


def _recipe_nan_negative(rng, B, M, C):
    conf = _scores(rng, B, M, C)
    z = rng.rand(B, M, C)
    conf[z < 0.15] = F(np.nan)
    conf[(z >= 0.15) & (z < 0.30)] = -conf[(z >= 0.15) & (z < 0.30)]
    return (conf,) + _groups(rng, B, M)


def _recipe_empty_class(rng, B, M, C):
    conf = _scores(rng, B, M, C)
    conf[:, :, 1] = rng.uniform(0, 0.05, (B, M)).astype(F)           # at or below the threshold 0.05
    return (conf,) + _groups(rng, B, M)


def _recipe_subnormal(rng, B, M, C):
    """Class 0: scores 1e-41 .. 1e-39 (subnormal; above threshold 0): s * x and the sums are subnormal too.  Class 1: scores 1.2e-38 ..
    2.4e-38 (normal) whose products with coordinates below 1 fall under 1.18e-38."""
    conf = _scores(rng, B, M, C, 0.01, 1.0)
    conf[:, :, 0] = (conf[:, :, 0] * F(1e-39)).astype(F)
    conf[:, :, 1] = (F(1.2e-38) + conf[:, :, 1] * F(1.2e-38)).astype(F)
    mn, mx = _groups(rng, B, M)
    mn, mx = (mn * F(0.05)).astype(F) + F(0.1), (mx * F(0.05)).astype(F) + F(0.1)
    tiny = np.finfo(F).tiny
    assert (conf[:, :, 0] > 0).all() and (conf[:, :, 0] < tiny).all() and (conf[:, :, 1] >= tiny).all()
    return conf, mn, mx


def _recipe_overflow_class0(rng, B, M, C):
    conf = _scores(rng, B, M, C)
    conf[:, 40:, 1] = F(0.0)                                            # class 1: forty candidates
    return (conf,) + _groups(rng, B, M)


def _recipe_classes_around_256(rng, B, M, C):
    conf = np.zeros((B, M, C), F)
    for c in CLASSES_AROUND_256:
        conf[:, :, c] = rng.uniform(0.06, 0.95, (B, M)).astype(F)
    return (conf,) + _groups(rng, B, M, 4)


RECIPES = {'classes_around_256': _recipe_classes_around_256, 'overlap': _recipe_overlap, 'groups': _recipe_groups, 'disjoint': _recipe_disjoint, 'tie_scores': _recipe_tie_scores,
           'zero_area': _recipe_zero_area, 'zeros': _recipe_zeros, 'nan_negative': _recipe_nan_negative, 'empty_class': _recipe_empty_class,
           'subnormal': _recipe_subnormal, 'overflow_class0': _recipe_overflow_class0}
HAND = ('hand2', 'hand3', 'fused_not_leader', 'score_tie', 'iou_tie', 't_above_v', 't_below_v', 'singleton_exact', 'clusters_fit', 'clusters_over',
        'rows_fit', 'rows_over')
NAMES = HAND + tuple(SEEDED)


@functools.lru_cache(maxsize=None)
def _hand_table():
    h = _hand()
    assert tuple(h) == HAND
    return h


@functools.lru_cache(maxsize=None)
def case(name):
    """{'name', 'B', 'M', 'C', 'thr', 'fuse_iou', 'V', 'max_per_class', 'R', 'conf' [B,M,C], 'xy_min', 'xy_max' [B,M,2]}: f32, read-only."""
    if name in HAND:
        conf, mn, mx, thr, fiou, V, P, R = _hand_table()[name]
    else:
        B, M, C, thr, fiou, V, P, R, recipe, seed = SEEDED[name]
        conf, mn, mx = RECIPES[recipe](np.random.RandomState(seed), B, M, C)
        R = M * C if R is None else R
    B, M, C = conf.shape
    assert mn.shape == mx.shape == (B, M, 2) and conf.dtype == mn.dtype == mx.dtype == F
    assert np.all(np.isfinite(mn)) and np.all(np.isfinite(mx)) and np.all(mn <= mx)
    # the kernel takes the thresholds as floats: what it compares with is the f32 value
    return {'name': name, 'B': B, 'M': M, 'C': C, 'thr': float(F(thr)), 'fuse_iou': float(F(fiou)), 'V': V, 'max_per_class': P, 'R': R,
            'conf': _frozen(conf), 'xy_min': _frozen(mn), 'xy_max': _frozen(mx)}


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = case(name)
    stats = []
    out = T.wbf(c['conf'], c['xy_min'], c['xy_max'], c['thr'], c['fuse_iou'], c['V'], c['max_per_class'], c['R'], stats)
    return tuple(_frozen(a) for a in out[:4]) + (out[4],), tuple(stats)


def reference(name):
    """The specification on a case: (out_conf [B,R,C], out_xy_min, out_xy_max [B,R,2], rows [B] int32, flags), read-only."""
    return _reference(name)[0]


def paths(name):
    """One dict per (image, class) that did not overflow: K (candidates), clusters, joins, T_max."""
    return _reference(name)[1]


# ---------------------------------------------------------------------------------------------------------------------
# the fusion restated box by box on one (image, class), with switches
# ---------------------------------------------------------------------------------------------------------------------

VARIANTS = ('leader_box', 'gt_iou', 'ties_high_index', 'iou_ties_high_cluster', 'singleton_divided', 'no_min', 'no_rescale')


def _iou(a, q):
    a1, a2 = (a[2] - a[0]) * (a[3] - a[1]), (q[2] - q[0]) * (q[3] - q[1])
    w = max(min(a[2], q[2]) - max(a[0], q[0]), F(0))
    h = max(min(a[3], q[3]) - max(a[1], q[1]), F(0))
    inter = w * h
    return inter / max((a1 + a2) - inter, F(1e-10))


def model(name, variant=None):
    """The fused (score, box) list of image 0, class 0 of a case, in emission order: [(f32, (f32,) * 4)].  `variant`: None or one of VARIANTS."""
    assert variant is None or variant in VARIANTS
    c = case(name)
    s, V = c['conf'][0, :, 0], c['V']
    box = np.concatenate([c['xy_min'][0], c['xy_max'][0]], 1)
    thr, fiou = F(c['thr']), F(c['fuse_iou'])
    cand = [i for i in range(len(s)) if s[i] > thr]
    cand.sort(key=lambda i: (-float(s[i]), -i if variant == 'ties_high_index' else i))
    clusters = []                                            # [leader box, fused box, sums, S, T]
    with np.errstate(all='ignore'):
        for i in cand:
            q, sc = box[i], s[i]
            best, best_iou = -1, None
            for k, cl in enumerate(clusters):
                v = _iou(cl[0] if variant == 'leader_box' else cl[1], q)
                if best < 0 or v > best_iou or (variant == 'iou_ties_high_cluster' and v == best_iou):
                    best, best_iou = k, v
            if best >= 0 and (best_iou > fiou if variant == 'gt_iou' else best_iou >= fiou):
                cl = clusters[best]
                cl[2] = [cl[2][k] + sc * q[k] for k in range(4)]
                cl[3] = cl[3] + sc
                cl[4] += 1
                cl[1] = [cl[2][k] / cl[3] for k in range(4)]
            else:
                sums = [sc * q[k] for k in range(4)]
                clusters.append([list(q), [sums[k] / sc for k in range(4)] if variant == 'singleton_divided' else list(q), sums, sc, 1])
        out = []
        for leader, fused, sums, S, n in clusters:
            if variant == 'no_rescale':
                score = S / F(n)
            else:
                score = ((S / F(n)) * F(n if variant == 'no_min' else min(n, V))) / F(V)
            assert isinstance(score, F) and all(isinstance(v, F) for v in fused)
            out.append((score, tuple(fused)))
    return out


def emitted(name):
    """The specification's rows of image 0 as model() lists them (a case with one class)."""
    oc, omn, omx, rows, _ = reference(name)
    return [(oc[0, r, 0], (omn[0, r, 0], omn[0, r, 1], omx[0, r, 0], omx[0, r, 1])) for r in range(rows[0])]


def same(a, b):
    """Two model() / emitted() lists, bit for bit."""
    return len(a) == len(b) and all(bits(F([x[0]] + list(x[1]))).tolist() == bits(F([y[0]] + list(y[1]))).tolist() for x, y in zip(a, b))
