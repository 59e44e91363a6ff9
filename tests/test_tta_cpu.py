"""tests/tta_ref.py (the specification of csrc/tta.hip), tests/tta_cases.py (the case table) and yolo_tf_amd/tta.py (the view list), without a
GPU: the hand-worked values, a wrong variant per rule that must differ where the case says it does, the gather identities, the overflow bits,
and the condition the single-view evaluation invariant relies on (a fusion of hard-NMS survivors at the same overlap changes nothing)."""
import numpy as np
import pytest

import soft_nms_ref as S
import tta_cases as C
import tta_ref as T
from yolo_tf_amd import tta

F = np.float32


def _rows(name):
    return [(float(s), tuple(float(v) for v in b)) for s, b in C.emitted(name)]


def test_hand_worked_values():
    assert _rows('hand2') == [(0.5, (0.0, 0.0, 4.0, 5.0))]
    assert _rows('hand3') == [(0.375, (0.0, 0.0, 4.0, 5.0))]
    for name in ('hand2', 'hand3'):
        oc, omn, omx, rows, flags = C.reference(name)
        assert rows.tolist() == [1] and flags == 0
        assert not C.bits(oc[0, 1:]).any() and not C.bits(omn[0, 1:]).any() and not C.bits(omx[0, 1:]).any()      # the tail is +0.0


@pytest.mark.parametrize('name', [n for n in C.NAMES if C.case(n)['C'] == 1 and C.case(n)['B'] == 1 and C.case(n)['M'] <= 300])
def test_model_restates_the_specification(name):
    if C.reference(name)[4] == 0:
        assert C.same(C.model(name), C.emitted(name))


# (case, the variant that must differ on it)
DISCRIMINATING = [('fused_not_leader', 'leader_box'), ('hand2', 'gt_iou'), ('score_tie', 'ties_high_index'), ('iou_tie', 'iou_ties_high_cluster'),
                  ('singleton_exact', 'singleton_divided'), ('t_above_v', 'no_min'), ('t_below_v', 'no_rescale')]


@pytest.mark.parametrize('name,variant', DISCRIMINATING)
def test_wrong_variant_differs(name, variant):
    right = C.model(name)
    assert C.same(right, C.emitted(name))
    assert not C.same(right, C.model(name, variant))


def test_every_variant_is_discriminated():
    assert {v for _, v in DISCRIMINATING} == set(C.VARIANTS)


def test_discriminating_cases_are_what_they_say():
    c = C.case('hand2')                                      # the overlap equals fuse_iou exactly
    box = np.concatenate([c['xy_min'][0], c['xy_max'][0]], 1)
    assert T.iou_clusters(box[:1], box[1])[0] == F(c['fuse_iou'])
    c = C.case('iou_tie')                                    # two clusters at the same overlap, which is fuse_iou
    box = np.concatenate([c['xy_min'][0], c['xy_max'][0]], 1)
    iou = T.iou_clusters(box[:2], box[2])
    assert iou[0] == iou[1] == F(c['fuse_iou'])
    assert len(C.emitted('iou_tie')) == 2 and C.emitted('iou_tie')[0][1] != tuple(box[0])      # cluster 0 took it
    assert len(C.emitted('fused_not_leader')) == 1 and len(C.model('fused_not_leader', 'leader_box')) == 2
    assert C.paths('t_above_v')[0]['T_max'] == 3 > C.case('t_above_v')['V'] and C.paths('t_below_v')[0]['T_max'] == 1 < C.case('t_below_v')['V']
    assert [r[1] for r in C.emitted('score_tie')] == [(0, 0, 2, 2), (4, 0, 6, 2)]


def test_singleton_search_is_bounded_and_exact():
    found = C.search_singleton(**C.SINGLETON_SEARCH)
    assert C.SINGLETON_SEARCH['draws'] <= 200 and found is not None
    _, s, x = found
    assert (s * x) / s != x
    (score, box), = C.emitted('singleton_exact')
    assert C.bits(F(box[2])) == C.bits(x) and C.bits(F(score)) == C.bits(s)      # V = 1, T = 1: (s / 1) * 1 / 1


def test_gather_flip_twice_is_the_identity_on_an_eighth_grid():
    rng = np.random.RandomState(5)
    w0 = 13
    x = np.sort(rng.randint(0, 8 * w0 + 1, (3, 40, 2)) / 8.0, axis=2).astype(F)
    y = np.sort(rng.randint(0, 8 * 13 + 1, (3, 40, 2)) / 8.0, axis=2).astype(F)
    mn, mx = np.stack([x[..., 0], y[..., 0]], -1), np.stack([x[..., 1], y[..., 1]], -1)
    conf = rng.uniform(0, 1, (3, 40, 4)).astype(F)
    once = T.gather_view(conf, mn, mx, F(1), F(1), w0, True)
    twice = T.gather_view(*once, F(1), F(1), w0, True)
    assert (once[1][..., 0] == F(w0) - mx[..., 0]).all() and (once[1] <= once[2]).all()
    for a, b in zip(twice, (conf, mn, mx)):
        assert (C.bits(a) == C.bits(b)).all()


def test_gather_scale_13_over_19():
    rng = np.random.RandomState(6)
    mn = rng.uniform(0, 9, (2, 30, 2)).astype(F)
    mx = (mn + rng.uniform(0.5, 9, (2, 30, 2))).astype(F)
    conf = rng.uniform(0, 1, (2, 30, 3)).astype(F)
    sx, sy = T.scales(13, 13, 19, 19)
    assert sx == F(13) / F(19) and sx.dtype == F
    for flip in (False, True):
        pc, pmn, pmx = T.gather([(conf, mn, mx, 13, 13, False), (conf, mn, mx, 19, 19, flip)], 13, 13)
        assert pc.shape == (2, 60, 3) and (C.bits(pmn[:, :30]) == C.bits(mn)).all() and (C.bits(pc[:, 30:]) == C.bits(conf)).all()
        k = F(13) / F(19)
        want_min = F(13) - mx[..., 0] * k if flip else mn[..., 0] * k
        want_max = F(13) - mn[..., 0] * k if flip else mx[..., 0] * k
        assert (C.bits(pmn[:, 30:, 0]) == C.bits(want_min)).all() and (C.bits(pmx[:, 30:, 0]) == C.bits(want_max)).all()
        assert (C.bits(pmn[:, 30:, 1]) == C.bits(mn[..., 1] * k)).all() and (C.bits(pmx[:, 30:, 1]) == C.bits(mx[..., 1] * k)).all()


def test_overflow_bits():
    for fit, over, bit in (('clusters_fit', 'clusters_over', T.FLAG_CLUSTERS), ('rows_fit', 'rows_over', T.FLAG_ROWS)):
        oc, _, _, rows, flags = C.reference(fit)
        assert flags == 0 and rows.tolist() == [8]
        oc, omn, omx, rows, flags = C.reference(over)
        assert flags == bit
        if bit == T.FLAG_CLUSTERS:                           # the (image, class) emits nothing
            assert rows.tolist() == [0] and not C.bits(oc).any() and not C.bits(omx).any()
        else:                                                # the image emits its first R
            assert rows.tolist() == [7] and (C.bits(oc[0, :, 0]) == C.bits(C.reference(fit)[0][0, :7, 0])).all()
    oc, _, _, rows, flags = C.reference('max_candidates_plus1')
    assert flags == T.FLAG_CANDIDATES and not C.bits(oc[0, :, 0]).any() and rows[0] > 0 and (oc[0, :rows[0], 1] > 0).all()
    assert C.reference('max_candidates')[4] == 0 and C.paths('max_candidates')[0]['K'] == T.MAX_CANDIDATES
    oc, _, _, rows, flags = C.reference('row_overflow_b3')
    assert flags == T.FLAG_ROWS and rows.tolist() == [20] * 3


def test_table_reaches_what_it_names():
    p = C.paths('dense')
    assert C.reference('dense')[4] == 0 and all(st['T_max'] >= 4 and st['joins'] > st['clusters'] for st in p)
    assert all(st['joins'] == 0 and st['clusters'] == st['K'] > 256 for st in C.paths('disjoint'))
    assert [st['K'] > 0 for st in C.paths('empty_class')] == [True, False, True] * 2
    assert all(st['clusters'] == 1 and st['K'] > 50 for st in C.paths('iou_zero'))
    assert all(st['joins'] == 0 for st in C.paths('iou_above_one'))
    c = C.case('nan_negative')
    assert np.isnan(c['conf']).any() and (c['conf'] < 0).any()
    assert all(st['K'] == int((c['conf'][st['b'], :, st['c']] > 0).sum()) for st in C.paths('nan_negative'))
    c = C.case('thr_zero')
    assert (C.bits(c['conf']) == 0x80000000).any() and (C.bits(c['conf']) == 0).any()
    c = C.case('zero_area')
    wh = c['xy_max'] - c['xy_min']
    assert ((wh[..., 0] == 0) & (wh[..., 1] == 0)).any()
    oc = C.reference('subnormal')[0]
    tiny = np.finfo(F).tiny
    assert ((oc[..., 0] > 0) & (oc[..., 0] < tiny)).any() and C.reference('subnormal')[4] == 0
    assert all(st['joins'] > 0 for st in C.paths('subnormal'))
    for name in C.NAMES:
        if name not in ('clusters_over', 'rows_over', 'max_candidates_plus1', 'row_overflow_b3'):
            assert C.reference(name)[4] == 0, name


def test_classes_beyond_one_emit_pass():
    c = C.case('c514_b2')
    assert c['C'] > 2 * 256 and [st['c'] for st in C.paths('c514_b2') if st['K'] > 0] == list(C.CLASSES_AROUND_256) * 2
    oc, _, _, rows, flags = C.reference('c514_b2')
    assert flags == 0 and (rows < c['R']).all()
    for b in range(2):
        cols = [int(np.flatnonzero(oc[b, r])[0]) for r in range(rows[b])]
        assert cols == sorted(cols) and set(cols) == set(C.CLASSES_AROUND_256)      # rows before, at and after both 256-class boundaries


def test_record_buffer_of_a_fused_evaluation():
    """A fused row is one (box, class): R records per image in either mode, which keeps a real dataset inside the evaluators' 2^31 - 1."""
    from yolo_tf_amd.evaluate import records_per_image
    n, M, Cn = 4952, 2 * (500 + 845 + 1805), 20             # VOC07 test under --tta "flip 320 608"
    R = tta.evaluation_rows(M, Cn)
    assert M == 6300 and R == 65536 == tta.ROWS_BOUND
    for mode in ('detect', 'all'):
        assert records_per_image(R, Cn, mode, 'voc', fused=True) == R
        assert n * records_per_image(R, Cn, mode, 'voc', fused=True) == 324534272 < 2 ** 31
        assert records_per_image(R, Cn, mode, 'coco', fused=True) == min(R, 100 * Cn) == 2000
    assert records_per_image(33800, 80, 'all', 'coco', fused=True) == 8000
    assert tta.evaluation_rows(1690, Cn) == 33800 and tta.evaluation_rows(130, Cn) == 2600 and tta.evaluation_rows(70000, 2) == 70000
    # without a fusion: what it was
    assert records_per_image(845, Cn, 'all') == 845 * Cn and records_per_image(845, Cn, 'detect') == 845
    assert records_per_image(845, Cn, 'all', 'coco') == 100 * Cn and records_per_image(845, Cn, 'detect', 'coco') == 845
    assert records_per_image(45, Cn, 'all', 'coco') == 45 * Cn


def test_parse_views():
    pv = tta.parse_views
    assert pv('', (416, 416), 32, 32) == [] and pv(None, (416, 416), 32, 32) == [] and pv(' , ', (416, 416), 32, 32) == []
    assert pv('flip', (416, 416), 32, 32) == [(416, 416, False), (416, 416, True)]
    assert pv('608 320', (416, 416), 32, 32) == [(416, 416, False), (320, 320, False), (608, 608, False)]
    assert pv('flip,320 416 608', (416, 416), 32, 32) == [(416, 416, False), (320, 320, False), (608, 608, False),
                                                        (416, 416, True), (320, 320, True), (608, 608, True)]
    assert pv('320 320x320 416 flip FLIP 320-352', (416, 416), 32, 32) == [(416, 416, False), (320, 320, False), (352, 352, False),
                                                                         (416, 416, True), (320, 320, True), (352, 352, True)]
    assert pv('416', (416, 416), 32, 32) == [(416, 416, False)]
    assert pv('96', (64, 96), 32, 32)[0] == (64, 96, False)
    with pytest.raises(ValueError, match="'mirror'"):
        pv('flip mirror', (416, 416), 32, 32)
    with pytest.raises(ValueError, match="'400'"):
        pv('400', (416, 416), 32, 32)
    views = pv('flip 320x416', (416, 416), 32, 32)
    assert tta.describe(views) == '416 320x416 416+flip 320x416+flip'
    assert tta.view_sizes(views) == [(416, 416), (320, 416)] and not tta.flip_only(views) and tta.flip_only(pv('flip', (416, 416), 32, 32))
    with pytest.raises(ValueError):
        tta.normalise([(416, 416, True)])
    with pytest.raises(ValueError):
        tta.normalise([(416, 416, False), (416, 416, False)])


@pytest.mark.parametrize('seed', range(8))
def test_fusion_of_hard_nms_survivors_changes_nothing(seed):
    """V = 1 and fuse_iou = the NMS overlap: every survivor is a cluster of its own and keeps its score and its box, bit for bit."""
    rng = np.random.RandomState(3000 + seed)
    B, N, Cn = 2, 150, 3
    thr, t = 0.05 if seed % 2 else 0.3, (0.45, 0.3, 0.6, 0.5)[seed % 4]
    conf = rng.uniform(0, 1, (B, N, Cn)).astype(F)
    mn, mx = C._boxes(rng, B, N)
    kept, _ = S.soft_nms(conf, mn, mx, thr, t, 'hard', with_order=False)
    oc, omn, omx, rows, flags = T.wbf(kept, mn, mx, thr, t, 1, 1024, N * Cn)
    assert flags == 0
    for b in range(B):
        got = {(int(np.flatnonzero(C.bits(oc[b, r]))[0]),) + tuple(C.bits(np.concatenate([oc[b, r][oc[b, r] != 0], omn[b, r], omx[b, r]])).tolist())
               for r in range(rows[b])}
        want = {(c,) + tuple(C.bits(np.concatenate([kept[b, i, c:c + 1], mn[b, i], mx[b, i]])).tolist())
                for i in range(N) for c in range(Cn) if kept[b, i, c] > F(thr)}
        assert len(got) == rows[b] == len(want) and got == want
        assert 0 < rows[b] < N * Cn
