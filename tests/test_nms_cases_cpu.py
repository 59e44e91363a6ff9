"""The NMS cases of tests/nms_cases.py, checked without a GPU: every case takes the kernel path its name claims and the table as a whole
reaches every path of csrc/nms.hip (the coverage table), the oracle's three implementations agree on every case, the restated kernel
algorithm equals the oracle bit for bit, and each way in which the kernel could be subtly wrong changes the result of some case (the
mutation table).  Run with -s to see the two tables."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import nms_cases as M
from oracle import yolo2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_ORACLE = os.path.join(ROOT, 'oracle', 'libnms_ref.so')
MUTATION_CASES = [n for n in M.NAMES if M.CASES[n][1] <= 1025 and M.CASES[n][0] * M.CASES[n][1] * M.CASES[n][2] <= 2 * 1025 * 3]       # (n2010 .. n4096, thr_neg1_n4096, eval_regime, c80_b3: the same paths, more time)


def _same(got, ref):
    """Scores as bit patterns and, where the case reports an order, the order."""
    return np.array_equal(M.bits(got[0]), M.bits(ref[0])) and (got[1] is None or np.array_equal(got[1], ref[1]))


# ---------------------------------------------------------------------------------------------------------------------
# the cases are what they say
# ---------------------------------------------------------------------------------------------------------------------

def _of(name, **where):
    return [p for p in M.paths(name) if all(p[k] == v for k, v in where.items())]


@pytest.mark.parametrize('name', M.NAMES)
def test_case_inputs_keep_the_contract(name):
    c = M.case(name)
    B, N, C = c['B'], c['N'], c['C']
    assert 1 <= N <= M.N_LIMIT and len(M.paths(name)) == B * C
    for k in ('conf', 'xy_min', 'xy_max'):
        assert c[k].dtype == np.float32 and not c[k].flags.writeable and np.all(np.isfinite(c[k]))
    assert np.all(c['xy_min'] <= c['xy_max'])
    assert c['thr'] == np.float32(c['thr']) and c['thr_iou'] == np.float32(c['thr_iou'])          # what the kernel receives is what the oracle gets
    if B > 1:
        assert not np.array_equal(c['conf'][0], c['conf'][1])                                      # different images
    for p in M.paths(name):
        negative = not (0.0 <= c['thr'])
        assert p['K'] == (N if negative else int((c['conf'][p['b'], :, p['c']] > np.float32(c['thr'])).sum()))
        assert p['full'] == (negative or (c['with_order'] and p['c'] == C - 1))
        assert p['groups'] == -(-p['K'] // 64) and p['chunks'] == -(-N // 64)
        assert p['np'] >= (N if p['full'] else p['K']) and p['np'] <= p['NP'] and p['np'] & (p['np'] - 1) == 0


@pytest.mark.parametrize('n', M.SIZES)
def test_size_cases(n):
    name = 'n%d' % n
    c = M.case(name)
    assert (c['B'], c['N'], c['C'], c['with_order']) == (2, n, 3, True)
    ps = M.paths(name)
    assert {p['full'] for p in ps if p['c'] == 2} == {True} and {p['full'] for p in ps if p['c'] < 2} == {False}
    assert all(p['per'] == -(-n // 256) for p in ps)
    if n >= 127:
        assert all(p['groups'] >= 2 and p['cross_group'] > 0 for p in ps)
    if n >= 63:
        assert all(p['tie_depth'] >= 1 for p in ps if p['c'] > 0)           # the repeated score ties in every class


def test_lds_boundary_pair():
    """The 64 KiB pair sits on the boundary of the formula restated in nms_cases.lds_bytes (from yolo2_nms): if the carve-up changes, this
    asks for the new pair."""
    assert M.lds_bytes(2010) == 65512 and M.lds_bytes(2011) == 65540
    assert M.lds_bytes(2010) <= M.LDS_DEFAULT < M.lds_bytes(2011)
    assert M.lds_bytes(4096) == 132112 <= 160 * 1024
    for n in range(1, M.N_LIMIT + 1):
        nchunks, NP = -(-n // 64), M.pow2_at_least(n, 2)
        assert 8 * (64 * nchunks + 1) <= 4 * n + 4 * NP + 1024               # the rows overlay fits the sort buffers at every size
        assert (M.lds_bytes(n) > M.LDS_DEFAULT) == (n >= 2011)               # one crossing


@pytest.mark.parametrize('k', M.COUNTS)
def test_candidate_count_cases(k):
    name = 'k%d' % k
    for b in range(2):
        p0, p1 = _of(name, b=b, c=0)[0], _of(name, b=b, c=1)[0]
        assert p0['K'] == k and p0['full'] is False and p0['np'] == M.pow2_at_least(k) and p0['groups'] == -(-k // 64)
        assert p1['full'] is True and p1['np'] == 512
        if k > 64:
            assert p0['cross_group'] > 0


def test_threshold_cases():
    assert all(p['full'] and p['K'] == 200 and p['alive'] > p['K'] - p['removed'] for p in M.paths('thr_neg1'))     # dead boxes suppressed too
    assert all(p['full'] and p['K'] == 4096 and p['groups'] == 64 and p['alive'] == 4095 for p in M.paths('thr_neg1_n4096'))   # every row is OR-ed in
    for name in ('thr_negzero', 'thr_zero'):
        c = M.case(name)
        zeros = (c['conf'] == 0).mean()
        assert 0.2 < zeros < 0.4 and np.signbit(c['conf'][c['conf'] == 0]).any() and not np.signbit(c['conf'][c['conf'] == 0]).all()
        assert not any(p['full'] for p in M.paths(name) if p['c'] < 2)
        assert np.signbit(M.reference(name)[0][M.reference(name)[0] == 0]).any()                # an untouched -0.0 keeps its sign
    assert np.signbit(np.float32(M.case('thr_negzero')['thr'])) and not np.signbit(np.float32(M.case('thr_zero')['thr']))
    c = M.case('eval_regime')
    assert (c['N'], c['C'], c['thr'], c['thr_iou']) == (845, 20, float(np.float32(0.005)), float(np.float32(0.45)))
    assert (c['conf'] == np.float32(0.005)).any() and 0.4 < (c['conf'] > np.float32(0.005)).mean() < 0.55
    c = M.case('thr_equals_score')
    assert 0.1 < (c['conf'] == np.float32(c['thr'])).mean() < 0.2
    c = M.case('thr_one')
    assert (c['conf'] == 1).any() and all(p['K'] == 0 for p in M.paths('thr_one'))
    assert np.array_equal(M.bits(M.reference('thr_one')[0]), M.bits(c['conf']))
    # IoU threshold 0: the best box of a class removes every other one
    out = M.reference('iou_zero')[0]
    assert np.all((out > np.float32(0.3)).sum(1) == 1)
    # IoU threshold 1: only exact duplicates go, and some do; above 1 nothing goes
    c, out = M.case('iou_one_dups'), M.reference('iou_one_dups')[0]
    boxes = np.concatenate([c['xy_min'][0], c['xy_max'][0]], 1)
    assert len(np.unique(boxes, axis=0)) == 40
    assert all(0 < p['removed'] for p in M.paths('iou_one_dups'))
    changed = np.argwhere(M.bits(out) != M.bits(c['conf']))
    assert len(changed) > 0
    assert np.array_equal(M.bits(M.reference('iou_above_one')[0]), M.bits(M.case('iou_above_one')['conf']))
    assert all(p['removed'] == 0 and p['alive'] == min(p['K'], 199) for p in M.paths('iou_above_one'))


def test_interface_cases():
    assert not any(p['full'] for p in M.paths('no_order')) and M.model('no_order')[1] is None
    assert [p['full'] for p in M.paths('c1')] == [True, True] and [p['full'] for p in M.paths('c1_no_order')] == [False, False]
    assert np.array_equal(M.bits(M.reference('c1')[0]), M.bits(M.reference('c1_no_order')[0]))
    c = M.case('c80_b3')
    assert (c['B'], c['C']) == (3, 80) and len(M.paths('c80_b3')) == 240
    assert M.SIDE_STREAM_CASE in M.CASES


def test_tie_cases():
    # tie_through_suppressed: in every motif Y (3m+1) is suppressed in class c-1, still sorts before X (3m) in class c and suppresses it
    c, (out, order) = M.case('tie_through_suppressed'), M.reference('tie_through_suppressed')
    for b, lo in ((0, 0), (1, 1)):
        x, y = np.arange(0, 96, 3), np.arange(1, 96, 3)
        assert np.all(c['conf'][b, x, lo + 1] == c['conf'][b, y, lo + 1]) and np.all(c['conf'][b, y, lo] > c['conf'][b, x, lo])
        assert np.all(out[b, y, lo] == 0) and np.all(out[b, x, lo] > 0)              # the mutated column would order them the other way
        assert np.all(out[b, x, lo + 1] == 0) and np.all(out[b, y, lo + 1] > 0)
    where = np.argsort(order[1])                                                     # box -> position in the reported order (image 1: class 2 ties)
    assert np.all(where[np.arange(1, 96, 3)] < where[np.arange(0, 96, 3)])
    assert max(p['tie_depth'] for p in M.paths('tie_chain3') if p['c'] == 4) == 3
    assert all(p['index_ties'] == 0 for p in M.paths('tie_chain3') if p['c'] == 4)
    assert all(p['index_ties'] > 0 and p['tie_depth'] == p['c'] for p in M.paths('tie_index'))


def test_geometry_cases():
    c = M.case('zero_area')
    wh = c['xy_max'] - c['xy_min']
    assert (wh[..., 0] == 0).any() and (wh[..., 1] == 0).any() and ((wh[..., 0] == 0) & (wh[..., 1] == 0)).any()
    points = np.concatenate([c['xy_min'][0], c['xy_max'][0]], 1)[2::4]
    assert len(np.unique(points, axis=0)) <= 4                                        # zero-area boxes identical to each other
    assert R.iou(points[0, :2], points[0, 2:], points[0, :2], points[0, 2:]) == 0     # 0 / 1e-10
    for name in ('at_threshold_straddle', 'at_threshold_straddle_no_order'):
        c, (out, order) = M.case(name), M.reference(name)
        for b in range(c['B']):
            seq = np.argsort(-c['conf'][b, :, 0], kind='stable')
            p, q = seq[63], seq[64]
            assert R.iou(c['xy_min'][b, p], c['xy_max'][b, p], c['xy_min'][b, q], c['xy_max'][b, q]) == np.float32(c['thr_iou'])
            assert out[b, q, 0] == 0 and (out[b, :, 0] == 0).sum() == 1               # `>=` fired, and only there
        assert all(p['K'] == 130 and p['cross_group'] == 1 for p in M.paths(name))


COVERAGE = {      # path -> (case, its paths) -> bool
    'full sort: last class with an order': lambda c, ps: c['thr'] >= 0 and any(p['full'] for p in ps),
    'full sort: every class (negative threshold)': lambda c, ps: not c['thr'] >= 0 and c['C'] > 1 and all(p['full'] for p in ps),
    'full sort: NP > N (padding)': lambda c, ps: any(p['full'] and p['NP'] > c['N'] for p in ps),
    'full sort: NP == N': lambda c, ps: any(p['full'] and p['NP'] == c['N'] for p in ps),
    'partial sort: K = 0': lambda c, ps: any(not p['full'] and p['K'] == 0 for p in ps),
    'partial sort: K = 1': lambda c, ps: any(not p['full'] and p['K'] == 1 for p in ps),
    'partial sort: K = np (no padding)': lambda c, ps: any(not p['full'] and p['K'] == p['np'] and p['K'] >= 64 for p in ps),
    'partial sort: K = np + 1': lambda c, ps: any(not p['full'] and p['K'] - 1 in (64, 128, 256) for p in ps),
    'partial sort: K = N': lambda c, ps: any(not p['full'] and p['K'] == c['N'] > 64 for p in ps),
    'partial sort of the last class (order_out = NULL)': lambda c, ps: not c['with_order'] and c['C'] > 1,
    'C = 1': lambda c, ps: c['C'] == 1,
    'scan: no pair (N = 1)': lambda c, ps: c['N'] == 1,
    'scan: one group of exactly 64': lambda c, ps: any(p['K'] == 64 for p in ps),
    'scan: removed words carried across groups': lambda c, ps: any(p['cross_group'] > 0 for p in ps),
    'scan: last 64-box word partly filled': lambda c, ps: c['N'] % 64 != 0 and any(p['groups'] > 1 for p in ps),
    'scan: last 64-box word full': lambda c, ps: c['N'] % 64 == 0 and any(p['groups'] > 1 for p in ps),
    'scan: 64 groups x 64 words (K = N = 4096)': lambda c, ps: any(p['groups'] == 64 and p['chunks'] == 64 and p['K'] == 4096 for p in ps),
    'scan: dead boxes suppress (negative threshold)': lambda c, ps: not c['thr'] >= 0 and any(p['alive'] > p['K'] - p['removed'] for p in ps),
    'count: two boxes per thread': lambda c, ps: ps[0]['per'] == 2,
    'LDS: request just below 64 KiB': lambda c, ps: M.LDS_DEFAULT - 64 < ps[0]['lds_bytes'] <= M.LDS_DEFAULT,
    'LDS: request just above 64 KiB': lambda c, ps: M.LDS_DEFAULT < ps[0]['lds_bytes'] <= M.LDS_DEFAULT + 64,
    'LDS: the largest request': lambda c, ps: ps[0]['lds_bytes'] == M.lds_bytes(M.N_LIMIT),
    'ties: broken three classes back': lambda c, ps: any(p['tie_depth'] >= 3 for p in ps),
    'ties: broken by the box index after every class': lambda c, ps: any(p['c'] >= 2 and p['index_ties'] > 0 for p in ps),
    'threshold -0.0': lambda c, ps: c['thr'] == 0 and np.signbit(np.float32(c['thr'])),
    'threshold 0.0': lambda c, ps: c['thr'] == 0 and not np.signbit(np.float32(c['thr'])),
    'threshold 0.005, IoU 0.45, 20 classes': lambda c, ps: c['name'] == 'eval_regime',
    'IoU threshold 0': lambda c, ps: c['thr_iou'] == 0,
    'IoU threshold 1': lambda c, ps: c['thr_iou'] == 1,
    'IoU threshold above 1': lambda c, ps: c['thr_iou'] > 1,
}


def test_every_path_is_reached_by_some_case():
    table = {path: [n for n in M.NAMES if hit(M.case(n), M.paths(n))] for path, hit in COVERAGE.items()}
    print('\npath coverage (%d cases)' % len(M.NAMES))
    for path, names in table.items():
        print('  %-52s %2d  %s' % (path, len(names), ' '.join(names[:8]) + (' ...' if len(names) > 8 else '')))
    assert not [path for path, names in table.items() if not names]


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's implementations agree; the restated kernel is the oracle
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', [n for n in M.NAMES if M.CASES[n][1] <= 130])
def test_fast_oracle_equals_the_literal_loop(name):
    c, ref = M.case(name), M.reference(name)
    conf = c['conf'].copy()
    for b in range(c['B']):
        order = R.non_max_suppress(conf[b].reshape(c['N'], 1, c['C']), c['xy_min'][b], c['xy_max'][b], c['thr'], c['thr_iou'])
        assert np.array_equal(order, ref[1][b])
    assert np.array_equal(M.bits(conf), M.bits(ref[0]))


@pytest.fixture(scope='module')
def c_oracle():
    """oracle/libnms_ref.so, built on the spot where it is missing (as tests/test_oracle.py _nms_lib does): a library that cannot be built
    fails these tests."""
    if not os.path.exists(C_ORACLE):
        subprocess.check_call(['make', '-C', os.path.join(ROOT, 'oracle')])
    lib = ctypes.CDLL(C_ORACLE)
    lib.nms_ref.restype = ctypes.c_int
    return lib


@pytest.mark.parametrize('name', M.NAMES)
def test_fast_oracle_equals_the_c_oracle(c_oracle, name):
    c, ref = M.case(name), M.reference(name)
    conf = c['conf'].copy()
    P = ctypes.POINTER(ctypes.c_float)
    for b in range(c['B']):
        order = np.zeros(c['N'], np.int64)
        rc = c_oracle.nms_ref(conf[b].ctypes.data_as(P), c['xy_min'][b].ctypes.data_as(P), c['xy_max'][b].ctypes.data_as(P), ctypes.c_long(c['N']),
                              ctypes.c_long(c['C']), ctypes.c_float(c['thr']), ctypes.c_float(c['thr_iou']), order.ctypes.data_as(ctypes.POINTER(ctypes.c_long)))
        assert rc == 0 and np.array_equal(order, ref[1][b])
    assert np.array_equal(M.bits(conf), M.bits(ref[0]))


@pytest.mark.parametrize('name', M.NAMES)
def test_restated_kernel_equals_the_oracle(name):
    """Also pins the claim of csrc/nms.hip's header: the order carried by the reference's stable sorts IS the lexicographic key on the
    original scores."""
    conf, order = M.model(name)
    ref = M.reference(name)
    assert np.array_equal(M.bits(conf), M.bits(ref[0]))
    assert (order is None) == (not M.case(name)['with_order'])
    if order is not None:
        assert np.array_equal(order, ref[1])


# ---------------------------------------------------------------------------------------------------------------------
# teeth: every way of being subtly wrong changes scores or order on some case
# ---------------------------------------------------------------------------------------------------------------------

_CAUGHT = {}


def caught(mutation):
    if mutation not in _CAUGHT:
        _CAUGHT[mutation] = [n for n in MUTATION_CASES if not _same(M.model(n, mutation), M.reference(n))]
    return _CAUGHT[mutation]


@pytest.mark.parametrize('mutation', M.MUTATIONS)
def test_every_mutation_is_caught_by_some_case(mutation):
    names = caught(mutation)
    print('\n  %-20s %2d  %s' % (mutation, len(names), ' '.join(names)))
    assert names


def test_mutations_are_caught_where_the_cases_were_built_for_them():
    assert 'tie_through_suppressed' in caught('ties_read_mutated')
    assert {'tie_chain3', 'tie_through_suppressed'} <= set(caught('index_ties'))
    assert 'thr_neg1' in caught('neg_thr_dead_stops') and set(caught('neg_thr_dead_stops')) == {'thr_neg1'}
    assert 'thr_neg1' not in caught('dead_suppresses') and 'n127' in caught('dead_suppresses')
    assert {'thr_equals_score', 'thr_zero', 'thr_negzero'} <= set(caught('lt_thr'))
    assert {'at_threshold_straddle', 'at_threshold_straddle_no_order'} <= set(caught('gt_iou'))
    assert {'at_threshold_straddle', 'at_threshold_straddle_no_order'} <= set(caught('contracted_union'))
    assert {'k129', 'k257', 'n129'} <= set(caught('group_local')) and not {'n63', 'n64', 'n65'} & set(caught('group_local'))       # (one group)
    assert 'k1' in caught('candidates_only')
