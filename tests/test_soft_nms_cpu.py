"""Soft-NMS without a GPU: soft_exp's accuracy, the specification (tests/soft_nms_ref.py) against the reference-pinned oracle and against
hand-built cases with exact results, the case table's coverage of the kernel's paths, a restatement whose mutations the table must catch,
the argument refusals of yolo2_soft_nms and the CLIs' flags.

The specification and the oracle (hard NMS).  The specification leaves every score that is not above the threshold untouched; the
reference's NMS (oracle.yolo2_ref.non_max_suppress_fast, and yolo2_nms) also writes +0 into such a box when it overlaps a kept one.  No
consumer can see the difference (they all test conf > threshold), but the bits differ, so the comparison here is: every CANDIDATE's score
bit for bit on every tie-free case; a non-candidate either as the oracle left it or untouched where the oracle wrote +0; and all bits
equal on the tie-free cases where the oracle touched no non-candidate (there must be some)."""
import configparser
import ctypes
import functools
import math

import numpy as np
import pytest

import soft_nms_cases as M
import soft_nms_ref as S
from oracle import yolo2_ref as R

F = np.float32
CEILING = 2.0 ** -21


# ---------------------------------------------------------------------------------------------------------------------
# soft_exp
# ---------------------------------------------------------------------------------------------------------------------

def test_soft_exp_accuracy_on_a_dense_sweep():
    """|soft_exp(x) / exp(x) - 1| <= 2^-21 on [-65, 0] against f64: four million evenly spaced points, every argument the Gaussian weight
    forms from a dyadic IoU and the sigmas of the case table, and the neighbourhoods of the reduction's rounding boundaries."""
    x = np.linspace(-65, 0, 4000001).astype(F)
    half = ((np.arange(-94, 1) + 0.5) * math.log(2)).astype(F)                  # where n = rint(x log2e) changes
    near = np.concatenate([np.nextafter(half, F(-100)), half, np.nextafter(half, F(0))])
    dyadic = -((np.arange(0, 1025) / F(1024)).astype(F) ** 2)[:, None] / F([1 / 64, 0.125, 0.5, 4])[None]
    x = np.concatenate([x, near[(near >= -65) & (near <= 0)], dyadic.astype(F).reshape(-1), F([-65, -64, -1, -0.5])])
    got = S.soft_exp(x).astype(np.float64)
    rel = np.abs(got / np.exp(x.astype(np.float64)) - 1)
    worst = int(np.argmax(rel))
    print('soft_exp: %d points, worst relative error %.3e = 2^%.2f at x = %r' % (len(x), rel[worst], math.log2(rel[worst]), float(x[worst])))
    assert rel[worst] <= CEILING
    assert np.all(got > 0) and np.all(got <= 1)                                   # a weight never raises a score


def test_soft_exp_of_zero_is_exactly_one():
    assert M.bits(S.soft_exp(F([0.0, -0.0]))).tolist() == [0x3F800000, 0x3F800000]
    # ... so a disjoint box (IoU 0, argument -(0 * 0 / sigma) = -0.0) keeps its bits under the Gaussian decay
    for sigma in (1 / 64, 0.5, 4):
        assert M.bits(S.weight(F([0.0]), 'gaussian', F(0.45), F(sigma))).tolist() == [0x3F800000]


def test_soft_exp_constants_are_the_headers():
    """csrc/soft_exp.h and tests/soft_nms_ref.py must spell the same f32 constants."""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'yolo_tf_amd', 'csrc', 'soft_exp.h')).read()
    text = re.sub(r'//.*', '', text)
    lits = [F(v) for v in re.findall(r'(-?\d+\.\d+(?:e-?\d+)?)f', text)]
    want = [S.LOG2E, S.LN2_HI, S.LN2_LO] + list(S.POLY)
    assert M.bits(F(lits)).tolist() == M.bits(F(want)).tolist()
    assert 'fma' not in text.lower() and 'exp(' not in text.replace('soft_exp(', '')


# ---------------------------------------------------------------------------------------------------------------------
# the specification against the oracle
# ---------------------------------------------------------------------------------------------------------------------

TIE_FREE = [n for n in M.NAMES if n != 'nan_scores' and M.tie_free(n)]


def test_the_table_has_tie_free_cases_of_every_kind():
    assert len(TIE_FREE) >= 30 and {'n1', 'n4096', 'chain4096', 'eval_regime', 'zero_area', 'dups5', 'c80_b3', 'thr_zero'} <= set(TIE_FREE)
    assert not M.tie_free('tie_index') and not M.tie_free('tie_by_decay')


@functools.lru_cache(maxsize=None)
def compare_with_oracle(name):
    """Asserts the comparison of the module docstring; returns whether the oracle touched a non-candidate."""
    c = M.case(name)
    spec, _ = M.reference(name, 'hard')
    oracle = c['conf'].copy()
    for b in range(c['B']):
        R.non_max_suppress_fast(oracle[b].reshape(c['N'], 1, c['C']), c['xy_min'][b], c['xy_max'][b], c['thr'], c['thr_iou'])
    cand = c['conf'] > F(c['thr'])
    sb, ob, ib = M.bits(spec), M.bits(oracle), M.bits(c['conf'])
    assert np.array_equal(sb[cand], ob[cand]), '%s: %d candidates differ' % (name, int((sb[cand] != ob[cand]).sum()))
    assert np.array_equal(sb[~cand], ib[~cand]), 'the specification touched a non-candidate'
    touched = ob[~cand] != ib[~cand]
    assert np.all(ob[~cand][touched] == 0), 'the oracle writes nothing but +0 into a non-candidate'
    if not touched.any():
        assert np.array_equal(sb, ob)
    return bool(touched.any())


@pytest.mark.parametrize('name', TIE_FREE)
def test_hard_specification_equals_the_oracle_on_tie_free_cases(name):
    compare_with_oracle(name)


def test_some_tie_free_cases_equal_the_oracle_in_every_bit():
    for name in ('chain4096', 'all_candidates', 'all_candidates_n257', 'disjoint'):
        assert name in TIE_FREE and not compare_with_oracle(name), name


# ---------------------------------------------------------------------------------------------------------------------
# hand-built cases: IoU exactly 1/2 and 1/4, exact dyadic results
# ---------------------------------------------------------------------------------------------------------------------

# A [0,0]-[2,1], B [0,0]-[1,1] (IoU(A, B) = 1/2), C [4,4]-[5,5] (apart)
THREE = (F([[0, 0], [0, 0], [4, 4]]), F([[2, 1], [1, 1], [5, 5]]), F([0.75, 0.5, 0.25]))
# A [0,0]-[2,2], B [0,0]-[1,1] (IoU(A, B) = 1/4), C [1,1]-[2,2] (IoU(A, C) = 1/4, apart from B and D), D [0,0]-[2,1] (IoU(A, D) = 1/2, IoU(B, D) = 1/2)
FOUR = (F([[0, 0], [0, 0], [1, 1], [0, 0]]), F([[2, 2], [1, 1], [2, 2], [2, 1]]), F([0.875, 0.5, 0.75, 0.625]))


def run(boxes, thr, thr_iou, method, sigma=0.5):
    mn, mx, s = boxes
    conf, order = S.soft_nms(s.reshape(1, -1, 1), mn[None], mx[None], thr, thr_iou, method, sigma)
    return conf[0, :, 0], order[0]


def test_hand_built_geometry():
    mn, mx, _ = FOUR
    area = (mx - mn).prod(1)
    assert S.iou_with(mn, mx, area, 0, np.arange(1, 4)).tolist() == [0.25, 0.25, 0.5]
    assert S.iou_with(mn, mx, area, 1, np.arange(2, 4)).tolist() == [0.0, 0.5] and S.iou_with(mn, mx, area, 2, np.array([3])).tolist() == [0.0]
    mn, mx, _ = THREE
    assert S.iou_with(mn, mx, (mx - mn).prod(1), 0, np.arange(1, 3)).tolist() == [0.5, 0.0]


def test_linear_three_boxes_exact():
    # A 0.75 is picked; B 0.5 x (1 - 1/2) = 0.25, now tied with C 0.25: the index picks B first; C is apart from both
    got, order = run(THREE, 0.125, 0.4, 'linear')
    assert got.tolist() == [0.75, 0.25, 0.25] and order.tolist() == [0, 1, 2]
    # threshold 0.25: B lands exactly on it and is not kept; C was never a candidate and keeps its bits
    got, order = run(THREE, 0.25, 0.4, 'linear')
    assert got.tolist() == [0.75, 0.0, 0.25] and M.bits(got)[1] == 0 and order.tolist() == [0, 2, 1]
    # threshold_iou above 1/2: nothing decays
    assert run(THREE, 0.125, 0.51, 'linear')[0].tolist() == [0.75, 0.5, 0.25]
    # hard: B goes
    assert run(THREE, 0.125, 0.5, 'hard')[0].tolist() == [0.75, 0.0, 0.25]


def test_linear_four_boxes_exact():
    # A 0.875; then B 0.5 x 3/4 = 0.375, C 0.75 x 3/4 = 0.5625 (IoU 1/4 >= 1/4 fires), D 0.625 x 1/2 = 0.3125; C is picked and touches nobody;
    # B is picked and halves D to 0.15625
    got, order = run(FOUR, 0.125, 0.25, 'linear')
    assert got.tolist() == [0.875, 0.375, 0.5625, 0.15625] and order.tolist() == [0, 2, 1, 3]
    got, order = run(FOUR, 0.1875, 0.25, 'linear')                   # D ends below the threshold: +0.0
    assert got.tolist() == [0.875, 0.375, 0.5625, 0.0] and order.tolist() == [0, 2, 1, 3]
    # threshold_iou just above 1/4: B and C keep their scores; C 0.75, then B 0.5, which halves D 0.3125 again
    got, order = run(FOUR, 0.125, float(np.nextafter(F(0.25), F(1))), 'linear')
    assert got.tolist() == [0.875, 0.5, 0.75, 0.15625] and order.tolist() == [0, 2, 1, 3]
    # re-selection matters: with scores that make D overtake B after A's pick, D is picked first and halves B
    mn, mx, _ = FOUR
    got, order = run((mn, mx, F([0.875, 0.25, 0.75, 0.4375])), 0.0625, 0.25, 'linear')
    # after A: B 0.1875, C 0.5625, D 0.21875; C; D 0.21875 (> B); B 0.1875 x 1/2 = 0.09375
    assert got.tolist() == [0.875, 0.09375, 0.5625, 0.21875] and order.tolist() == [0, 2, 3, 1]


def f64_soft_nms(boxes, thr, sigma):
    """Gaussian Soft-NMS in f64 with math.exp: (final scores, the number of weights other than 1 that went into each)."""
    mn, mx, s = (np.asarray(a, np.float64) for a in boxes)
    s = s.copy()
    n = len(s)
    factors = np.zeros(n, int)
    live = set(range(n))
    out = np.zeros(n)

    def iou(i, j):
        wh = np.maximum(np.minimum(mx[i], mx[j]) - np.maximum(mn[i], mn[j]), 0)
        inter = wh[0] * wh[1]
        return inter / ((mx[i] - mn[i]).prod() + (mx[j] - mn[j]).prod() - inter)
    while live:
        m = max(live, key=lambda i: (s[i], -i))
        if not s[m] > thr:
            break
        live.remove(m)
        out[m] = s[m]
        for j in live:
            v = iou(m, j)
            if v > 0:
                s[j] *= math.exp(-v * v / sigma)
                factors[j] += 1
    return out, factors


@pytest.mark.parametrize('boxes', [THREE, FOUR], ids=['three', 'four'])
@pytest.mark.parametrize('sigma', [0.5, 0.125, 4.0])
def test_gaussian_hand_built_against_f64(boxes, sigma):
    thr = 0.01
    got, order = run(boxes, thr, 0.4, 'gaussian', sigma)
    want, factors = f64_soft_nms(boxes, thr, sigma)
    assert factors.max() >= (2 if len(boxes[2]) == 4 else 1) and np.all(want > thr)
    for g, w, k in zip(got.astype(np.float64), want, factors):
        if k == 0:
            assert g == w                                             # only weights of exactly 1: the score's bits are kept
        else:
            assert abs(g / w - 1) <= CEILING * k
    assert order.tolist() == sorted(range(len(want)), key=lambda i: (-want[i], i))


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------

def test_cases_are_read_only_and_cached():
    c = M.case('n65')
    assert M.case('n65') is c and M.reference('n65', 'linear')[0] is M.reference('n65', 'linear')[0]
    for a in (c['conf'], c['xy_min'], c['xy_max'], M.reference('n65', 'linear')[0], M.reference('n65', 'linear')[1]):
        with pytest.raises(ValueError):
            a[...] = 0


def test_the_table_has_the_sizes_counts_and_parameters():
    sizes = {M.CASES[n][1] for n in M.NAMES}
    assert {1, 2, 63, 64, 65, 255, 256, 257, 513, 845, 1025, 2727, 2728, 4095, 4096} <= sizes
    for k in M.COUNTS:
        for st in M.paths('k%d' % k, 'linear'):
            if st['c'] == 0:
                assert st['K'] == k
    for name in ('all_candidates', 'all_candidates_n257', 'chain4096'):
        assert all(st['K'] == st['N'] for st in M.paths(name, 'gaussian'))
    c = M.case('chain4096')
    assert (c['B'], c['N'], c['C']) == (1, 4096, 1)
    for method in ('linear', 'gaussian'):
        assert M.paths('chain4096', method)[0]['picks'] == 4096                # the longest chain
    assert M.case('eval_regime')['conf'].shape == (2, 845, 20) and (M.case('eval_regime')['thr'], M.case('eval_regime')['thr_iou']) == (float(F(0.005)), float(F(0.45)))
    assert {M.case(n)['thr_iou'] for n in M.NAMES} >= {0.0, 1.0, 1.5}
    assert {M.case(n)['sigma'] for n in M.NAMES} >= {1 / 64, 0.5, 4.0}
    assert {M.case(n)['C'] for n in M.NAMES} >= {1, 80} and 3 in {M.case(n)['B'] for n in M.NAMES}
    assert not M.case('no_order')['with_order'] and M.SIDE_STREAM_CASE in M.NAMES
    z = M.case('thr_zero')
    assert z['thr'] == 0.0 and (M.bits(z['conf']) == 0x80000000).any() and (M.bits(z['conf']) == 0).any()
    e = M.case('thr_equals_score')
    assert (e['conf'] == F(e['thr'])).mean() > 0.1
    assert np.isnan(M.case('nan_scores')['conf']).any()


def test_the_table_reaches_every_path_of_the_kernel():
    every = {m: [st for n in M.NAMES for st in M.paths(n, m)] for m in ('linear', 'gaussian')}
    for m, sts in every.items():
        assert {0, 1, 2, 64, 65, 256, 257, 4096} <= {st['K'] for st in sts}
        assert {0, 1, 2, 16} <= {st['per'] for st in sts}, 'positions per thread in the pick loop'
        assert {1, 2, 16} <= {st['chunks_per_wave'] for st in sts} and {1, 2} <= {st['chunks'] for st in sts}
        assert {False, True} == {st['lds_raised'] for st in sts}
        assert {2, 64, 128, 256, 512, 1024, 2048, 4096} <= {st['NP'] for st in sts}
        assert any(st['zeroed'] for st in sts) and any(st['K'] and st['picks'] == st['K'] for st in sts)
        assert any(st['subnormal'] for st in M.paths('subnormal', m)), m
        assert any(st['floor'] for st in M.paths('zero_area', m))
    assert sum(st['decay_ties'] for st in M.paths('tie_by_decay', 'linear')) > 0
    # waves without a candidate, and waves without a box: N = 65 gives wave 0 both chunks; K = 1 leaves three waves empty
    assert M.paths('n65', 'linear')[0]['chunks_per_wave'] == 1 and M.paths('n65', 'linear')[0]['chunks'] == 2


def test_landing_on_the_threshold():
    """In both landing cases the decay of the method they are built for leaves scores exactly at the threshold (written as +0), just
    below it (+0) and just above it (kept)."""
    for name, method in (('land_linear', 'linear'), ('land_gaussian', 'gaussian')):
        c = M.case(name)
        thr = F(c['thr'])
        mn, mx = c['xy_min'][0], c['xy_max'][0]
        area = (mx - mn).prod(1)
        big = np.flatnonzero(area == 2)
        landed = []
        for a in big:
            js = np.flatnonzero((area == 1) & (np.abs(mn[:, 0] - mn[a, 0]) < 3) & (np.abs(mn[:, 1] - mn[a, 1]) < 3))
            assert len(js) == 2
            iou = S.iou_with(mn, mx, area, a, js)
            assert iou.tolist() == [0.5, 0.5]
            landed += (c['conf'][0, js, 0] * S.weight(iou, method, F(c['thr_iou']), F(c['sigma']))).tolist()
        landed = F(landed)
        assert (landed == thr).sum() >= 10 and (landed < thr).sum() >= 10 and (landed > thr).sum() >= 10
        out = M.reference(name, method)[0][0, :, 0]
        small = np.flatnonzero(area == 1)
        kept = out[small] > thr
        assert kept.sum() == (landed > thr).sum() and np.all(M.bits(out[small][~kept]) == 0)


def test_disjoint_boxes_keep_every_bit():
    for method in S.METHODS:
        assert np.array_equal(M.bits(M.reference('disjoint', method)[0]), M.bits(M.case('disjoint')['conf']))


def test_duplicates_decay_by_the_exact_weights():
    """Five-fold duplicates, IoU exactly 1: the linear weight is exactly 0, the Gaussian one soft_exp(-1 / sigma)."""
    c = M.case('dups5')
    assert S.weight(F([1.0]), 'linear', F(c['thr_iou']), F(c['sigma'])).tolist() == [0.0]
    assert M.bits(S.weight(F([1.0]), 'gaussian', F(0), F(0.5))).tolist() == M.bits(S.soft_exp(F([-2.0]))).tolist()
    assert M.bits(S.weight(F([1.0]), 'gaussian', F(0), F(1 / 64))).tolist() == M.bits(S.soft_exp(F([-64.0]))).tolist()
    mn, mx = c['xy_min'][0], c['xy_max'][0]
    _, inverse, counts = np.unique(np.concatenate([mn, mx], 1), axis=0, return_inverse=True, return_counts=True)
    assert np.all(counts == 5)
    lin = M.reference('dups5', 'linear')[0][0]
    for k in range(c['C']):
        for g in range(len(counts)):
            members = np.flatnonzero(inverse.reshape(-1) == g)
            assert (lin[members, k] > F(c['thr'])).sum() <= 1          # at most one of five identical boxes survives the linear decay


def test_nan_scores_are_no_candidates():
    c = M.case('nan_scores')
    nan = np.isnan(c['conf'])
    for method in S.METHODS:
        out = M.reference('nan_scores', method)[0]
        assert np.array_equal(M.bits(out)[nan], M.bits(c['conf'])[nan]) and not np.isnan(out[~nan]).any()


# ---------------------------------------------------------------------------------------------------------------------
# the restatement and its mutations
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('method', S.METHODS)
def test_the_restated_algorithm_equals_the_specification_everywhere(method):
    for name in M.NAMES:
        if method == 'hard' and M.CASES[name][1] > 1100:
            continue                                                   # (the large hard cases are the oracle comparison's)
        conf, order = M.model(name, method)
        ref_conf, ref_order = M.reference(name, method)
        assert np.array_equal(M.bits(conf), M.bits(ref_conf)), (name, method)
        assert order is None and ref_order is None or np.array_equal(order, ref_order), (name, method)


@pytest.mark.parametrize('mutation', M.MUTATIONS)
def test_every_mutation_is_caught_by_some_case(mutation):
    caught = [(n, m) for n in M.SMALL for m in ('linear', 'gaussian', 'hard')
              if not np.array_equal(M.bits(M.model(n, m, mutation)[0]), M.bits(M.reference(n, m)[0]))]
    print('%s: caught by %d (case, method) pairs, e.g. %s' % (mutation, len(caught), caught[:6]))
    assert caught
    if mutation != 'gt_iou':                                           # (`>` for `>=` has no meaning for the Gaussian weight)
        assert {m for _, m in caught} >= {'linear', 'gaussian'}, 'each soft method must catch it'
    else:
        assert {m for _, m in caught} >= {'linear'}


# ---------------------------------------------------------------------------------------------------------------------
# the entry point's refusals and the CLIs
# ---------------------------------------------------------------------------------------------------------------------

GOOD = dict(B=1, N=16, C=2, method=2, thr=0.3, thr_iou=0.45, sigma=0.5)


@pytest.mark.parametrize('bad', [dict(method=3), dict(method=-1), dict(thr=-0.1), dict(thr=float('nan')), dict(thr_iou=float('inf')),
                                 dict(thr_iou=float('nan')), dict(sigma=1 / 128), dict(sigma=0.0), dict(sigma=float('nan')), dict(sigma=float('inf')),
                                 dict(N=0), dict(N=4097), dict(B=0), dict(C=0), dict(conf=None), dict(xy_min=None), dict(xy_max=None)],
                         ids=lambda d: '%s=%s' % next(iter(d.items())))
def test_argument_errors_raise_without_touching_the_gpu(bad):
    """YOLO2_E_ARG before any HIP call: the pointers are host addresses that a launch would fault on, and no GPU is needed."""
    from yolo_tf_amd import _lib
    host = (ctypes.c_float * 4096)()
    a = dict(GOOD, conf=ctypes.addressof(host), xy_min=ctypes.addressof(host), xy_max=ctypes.addressof(host))
    a.update(bad)
    with pytest.raises(_lib.HipKernelError, match='argument check failed'):
        _lib.call('yolo2_soft_nms', a['conf'], a['xy_min'], a['xy_max'], None, a['B'], a['N'], a['C'], a['method'], a['thr'], a['thr_iou'], a['sigma'], None)


def test_method_constants_match_the_header():
    import os
    import re
    from yolo_tf_amd import _lib, utils
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'yolo2_hip.h')).read()
    header = {k.lower(): int(v) for k, v in re.findall(r'#define YOLO2_NMS_(HARD|LINEAR|GAUSSIAN) (\d+)', text)}
    assert header == _lib.NMS_METHODS == {'hard': 0, 'linear': 1, 'gaussian': 2}
    assert tuple(_lib.NMS_METHODS) == utils.NMS_METHODS == S.METHODS
    assert _lib.query('yolo2_abi_version') == 1


def test_ops_soft_nms_refuses_an_unknown_method_name():
    from yolo_tf_amd import ops
    with pytest.raises(ValueError):
        ops.soft_nms(None, None, None, None, 1, 16, 2, 'softer', 0.3, 0.45, 0.5)


def test_both_clis_accept_the_flags_and_default_to_hard():
    import detect as detect_cli
    import eval as eval_cli
    from yolo_tf_amd import utils
    empty = configparser.ConfigParser()
    ini = configparser.ConfigParser()
    ini.read_string('[mi355x]\nnms = linear\nnms_sigma = 0.25\n')
    for make, lead in ((detect_cli.make_args, ['image.jpg']), (eval_cli.make_args, [])):
        args = make(lead)
        assert utils.nms_options(args, empty) == ('hard', 0.5)
        assert utils.nms_options(args, ini) == ('linear', 0.25)                  # [mi355x] nms / nms_sigma
        args = make(lead + ['--nms', 'gaussian', '--sigma', '0.75'])
        assert (args.nms, args.sigma) == ('gaussian', 0.75)
        assert utils.nms_options(args, ini) == ('gaussian', 0.75)                # the flag wins
        assert utils.nms_options(make(lead + ['--nms', 'hard']), ini) == ('hard', 0.25)
        with pytest.raises(SystemExit):
            make(lead + ['--nms', 'softer'])
    bad = configparser.ConfigParser()
    bad.read_string('[mi355x]\nnms = softer\n')
    with pytest.raises(ValueError):
        utils.nms_options(eval_cli.make_args([]), bad)
