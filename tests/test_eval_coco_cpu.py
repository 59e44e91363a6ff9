"""Hand-worked examples that pin the COCO checker (tests/coco_ref.py) to the rules of include/yolo2_hip.h, section "evaluation, COCO
protocol".  Every expected value is derived in a comment.  Tolerance 1e-12: the sums have at most 101 f64 terms of at most 1, and a
precision of "1" is 1 / (1 + 2.2e-16)."""
import numpy as np

import coco_ref

TOL = 1e-12


def run(dets, gts, C=1, **kw):
    """One image with scale 1 (cells = pixels).  dets: [(box, class, score)]; gts: [(box, class, flags)] or [(box, class, flags, area)]
    (default area: the box's).  Returns (records, npig, result of evaluate)."""
    N = max(len(dets), 1)
    conf = np.zeros((1, N, C), np.float32)
    boxes = np.zeros((1, N, 4), np.float32)
    for i, (bx, c, s) in enumerate(dets):
        boxes[0, i], conf[0, i, c] = bx, s
    gb = np.asarray([g[0] for g in gts], np.float32).reshape(-1, 4)
    area = np.asarray([g[3] if len(g) > 3 else (g[0][2] - g[0][0]) * (g[0][3] - g[0][1]) for g in gts], np.float32)
    recs, npig = coco_ref.collect(conf, boxes[..., :2], boxes[..., 2:], np.asarray([g[1] for g in gts], np.int32), gb, area,
                                  np.asarray([g[2] for g in gts], np.uint8), np.array([0, len(gts)], np.int32), np.ones((1, 2), np.float32), 0, 1, 0.01,
                                  'all', **kw)
    return recs, npig, coco_ref.evaluate(recs, npig, C)


def close(a, b):
    return abs(a - b) <= TOL


def test_perfect_detections_give_one_everywhere():
    # one box per class, of area 10^2 (small), 50^2 (medium), 100^2 (large); each detection equals its box: one TP per class at every
    # threshold, precision 1 at recall 1, so every AP and recall that has ground truth is 1 and the rest is -1 and left out
    gts = [([0, 0, 10, 10], 0, 0), ([0, 0, 50, 50], 1, 0), ([0, 0, 100, 100], 2, 0)]
    recs, npig, res = run([(g[0], g[1], 0.9) for g in gts], gts, C=3)
    assert npig.tolist() == [[1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert all(close(v, 1.0) for v in res['stats'])
    assert (res['ap'][3, :, 1:] == -1).all() and (np.abs(res['ap'][2] - 1) <= TOL).all()


def test_one_tp_then_one_fp_with_two_boxes():
    # two boxes, the better detection hits the first, the other one nothing: tp = 1 1, fp = 0 1, recall .5 .5, precision 1 .5.  The 51
    # recall thresholds 0, .01 .. .50 are reached at index 0 (precision 1), the other 50 never: AP = 51/101, recall .5
    gts = [([0, 0, 10, 10], 0, 0), ([50, 50, 60, 60], 0, 0)]
    recs, npig, res = run([([0, 0, 10, 10], 0, 0.9), ([200, 200, 210, 210], 0, 0.8)], gts)
    assert npig[0, 0] == 2
    assert close(res['ap'][2, 0, 0], 51 / 101) and close(res['recall'][2, 0, 0], 0.5)
    assert close(res['stats'][1], 51 / 101)


def test_a_free_box_that_counts_wins_over_a_better_ignored_one():
    # the detection overlaps an ignored box at 80/100 and a free box that counts at 60/100.  Boxes that count are scanned first and the
    # scan stops at the first ignored box once something matched: at t = .5 and .55 the match is the box that counts (VOC's rule would
    # pick the best overlap and ignore the detection).  At t = .65 and .7 only the ignored box overlaps enough: matched and ignored
    gts = [([4, 4, 14, 12], 0, 1), ([4, 4, 10, 14], 0, 0)]
    recs, npig, res = run([([4, 4, 14, 14], 0, 0.9)], gts)
    m, ig = recs[0]['matched'], recs[0]['ignored']
    assert m[0, :2].all() and not ig[0, :2].any()
    assert m[0, 3:5].all() and ig[0, 3:5].all()
    assert not m[0, 8:].any() and not ig[0, 8:].any()          # t >= .9: nothing overlaps enough; area 100 is inside "all": a false positive
    assert close(res['ap'][2, 0, 0], 1.0)


def test_of_equal_overlaps_the_later_box_wins():
    # both boxes overlap the first detection at 80/100.  >= keeps the LATER one (index 1).  The second detection equals box 0: it is
    # still free, overlap 1, a match at t = .75.  Had the first detection taken box 0, the second would see box 1 at 60/100 only
    gts = [([0, 0, 10, 8], 0, 0), ([0, 2, 10, 10], 0, 0)]
    recs, _, _ = run([([0, 0, 10, 10], 0, 0.9), ([0, 0, 10, 8], 0, 0.8)], gts)
    assert [r['rank'] for r in recs] == [0, 1]
    assert recs[0]['matched'][0, 5] and recs[1]['matched'][0, 5] and recs[1]['matched'][0, 9]


def test_an_overlap_equal_to_the_threshold_matches():
    # intersection 1, union 2 on integer coordinates: IoU is float32(.5) exactly, and a match needs only iou >= t (VOC: strictly above)
    gts = [([1, 1, 2, 2], 0, 0)]
    recs, _, res = run([([1, 1, 3, 2], 0, 0.75)], gts)
    assert recs[0]['matched'][0, 0] and not recs[0]['matched'][0, 1]
    assert close(res['ap'][2, 0, 0], 1.0) and res['ap'][2, 1, 0] == 0.0


def test_detections_inside_a_crowd_box_are_all_ignored():
    # against a crowd box the overlap is intersection / detection area = 1 for a detection inside it, and a crowd box can be taken
    # again: all three match it and are ignored everywhere.  The crowd box does not count as ground truth; the other box does
    gts = [([0, 0, 100, 100], 0, 2), ([300, 300, 310, 310], 0, 0)]
    recs, npig, res = run([([10, 10, 20, 20], 0, 0.9), ([30, 30, 40, 40], 0, 0.8), ([50, 50, 70, 70], 0, 0.7)], gts)
    assert len(recs) == 3 and all(r['matched'].all() and r['ignored'].all() for r in recs)
    assert npig[:, 0].tolist() == [1, 1, 0, 0]
    assert res['ap'][2, 0, 0] == 0.0 and res['recall'][2, 0, 0] == 0.0          # ground truth, no counted detection


def test_a_second_detection_on_a_taken_box_takes_the_next_best_free_one():
    # detection 0 equals box 0.  Detection 1 overlaps box 0 at 90/100 (taken) and box 1 at 70/90 = .777: it falls through to box 1, a
    # second TP at t <= .75 (VOC: a duplicate, FP).  At t = .8 box 1 is not enough: FP
    gts = [([0, 0, 10, 10], 0, 0), ([0, 0, 10, 7], 0, 0)]
    recs, _, res = run([([0, 0, 10, 10], 0, 0.9), ([0, 0, 10, 9], 0, 0.8)], gts)
    assert recs[1]['matched'][0, :6].all() and not recs[1]['matched'][0, 6:].any()
    assert close(res['ap'][2, 0, 0], 1.0) and close(res['recall'][2, 0, 0], 1.0)
    # t = .8: tp = 1 1, fp = 0 1 of 2 boxes, as in the second example
    assert close(res['ap'][2, 6, 0], 51 / 101) and close(res['recall'][2, 6, 0], 0.5)


def test_an_unmatched_detection_is_ignored_outside_its_area_range():
    # area 20^2 = 400: inside "all" [0, 1e10] and "small" [0, 1024], outside "medium" and "large"
    gts = [([300, 300, 310, 310], 0, 0)]
    recs, _, _ = run([([0, 0, 20, 20], 0, 0.9)], gts)
    assert not recs[0]['matched'].any()
    assert recs[0]['ignored'].tolist() == [[False] * 10, [False] * 10, [True] * 10, [True] * 10]


def test_the_detection_limit_keeps_the_first_ranks_only():
    # three boxes, three perfect detections in one image: under the limit 1 only rank 0 counts, recall 1/3; under 10 all do
    gts = [([0, 0, 10, 10], 0, 0), ([20, 20, 30, 30], 0, 0), ([40, 40, 50, 50], 0, 0)]
    recs, _, res = run([(g[0], 0, s) for g, s in zip(gts, (0.9, 0.8, 0.7))], gts)
    assert close(res['recall'][0, 0, 0], 1 / 3) and close(res['recall'][1, 0, 0], 1.0)
    assert close(res['stats'][6], 1 / 3) and close(res['stats'][7], 1.0)
    # max_dets = 2: the third detection makes no record at all
    assert [r['rank'] for r in run([(g[0], 0, s) for g, s in zip(gts, (0.9, 0.8, 0.7))], gts, max_dets=2)[0]] == [0, 1]


def test_a_class_without_ground_truth_is_left_out():
    # class 1 has a detection and no box: -1 everywhere, and the means are those of class 0 alone (a perfect detection: 1)
    gts = [([0, 0, 10, 10], 0, 0)]
    _, _, res = run([([0, 0, 10, 10], 0, 0.9), ([0, 0, 10, 10], 1, 0.9)], gts, C=2)
    assert (res['ap'][:, :, 1] == -1).all() and (res['recall'][:, :, 1] == -1).all()
    assert close(res['stats'][0], 1.0) and close(res['stats'][8], 1.0)
    assert res['stats'][4] == -1.0 and res['stats'][5] == -1.0              # no medium or large box at all


def test_the_evaluators_stats_equal_the_checkers():
    # the twelve numbers are means over the entries that are not -1; -1 when nothing is left or the table lacks the threshold
    from yolo_tf_amd import evaluate
    rng = np.random.RandomState(0)
    ap, recall = rng.uniform(size=(6, 10, 7)), rng.uniform(size=(6, 10, 7))
    ap[:, :, 2] = recall[:, :, 2] = -1
    ap[4] = recall[4] = -1                                  # no medium box at all
    slices = evaluate.coco_slices(4, 100)
    assert slices == coco_ref.SLICES
    got = evaluate.coco_stats(ap, recall, coco_ref.IOU_THRESHOLDS, slices)
    want = coco_ref.stats(ap, recall)
    assert got[4] == -1 and got[10] == -1 and all(close(a, b) for a, b in zip(got, want))
    assert close(got[1], ap[2, 0][ap[2, 0] > -1].mean()) and close(got[2], ap[2, 5][ap[2, 5] > -1].mean())
    assert evaluate.coco_stats(ap[:, :3], recall[:, :3], [0.5, 0.6, 0.7], slices)[2] == -1          # no threshold .75 in the table
    assert len(evaluate.COCO_STAT_NAMES) == 12


def test_load_npz_reads_the_optional_crowd_and_area(tmp_path):
    from yolo_tf_amd import evaluate
    images = np.empty(2, object)
    images[0], images[1] = np.zeros((8, 9, 3), np.uint8), np.zeros((5, 6, 3), np.uint8)
    base = dict(images=images, objects_class=np.array([1, 2, 3]), objects_coord=np.arange(12, dtype=np.float32).reshape(3, 4), objects_first=np.array([0, 2, 3]))
    np.savez(str(tmp_path / 'a.npz'), **base)
    np.savez(str(tmp_path / 'b.npz'), objects_crowd=np.array([0, 1, 0]), objects_area=np.array([5.0, 6.0, 7.0]), **base)
    assert len(evaluate.load_npz(str(tmp_path / 'b.npz'))) == 3                     # the VOC layout is what it was
    _, _, difficult, crowd, area = evaluate.load_npz(str(tmp_path / 'a.npz'), coco=True)
    assert [c.tolist() for c in crowd] == [[0, 0], [0]] and area is None and [d.tolist() for d in difficult] == [[0, 0], [0]]
    _, objects, _, crowd, area = evaluate.load_npz(str(tmp_path / 'b.npz'), coco=True)
    assert [c.tolist() for c in crowd] == [[0, 1], [0]] and [a.tolist() for a in area] == [[5.0, 6.0], [7.0]] and objects[1][0].tolist() == [3]


def test_eval_py_takes_the_protocol():
    import importlib
    mod = importlib.import_module('eval')
    assert mod.make_args([]).protocol == 'voc' and mod.make_args(['--protocol', 'coco']).protocol == 'coco'


def test_size_queries_and_argument_checks_need_no_gpu():
    import ctypes
    import pytest
    from yolo_tf_amd import _lib
    from yolo_tf_amd.evaluate import COCO_RECORD_DTYPE
    q = _lib.query
    up = lambda n: (n + 255) // 256 * 256
    assert COCO_RECORD_DTYPE.itemsize == 40 and q('yolo2_eval_coco_record_bytes', 1000) == 40 * 1000 and q('yolo2_eval_coco_record_bytes', 0) == 0
    assert q('yolo2_eval_coco_result_bytes', 6, 10, 4, 80) == 8 * (2 * 6 * 10 * 80 + 4 * 80 + 3)
    assert q('yolo2_eval_coco_workspace_bytes', 1000, 20) == 2 * 16128 + 1024           # two buffers of 16-byte keys + one tile's digit table
    B, N, C = 64, 845, 20                                   # counts, per-class counts and prefixes, per-box class and score, 4 key rows per image
    assert q('yolo2_eval_coco_collect_workspace_bytes', B, N, C) == up(4 * B) + 2 * up(4 * B * C) + 2 * up(4 * B * N) + up(8 * 4 * B * N)
    assert q('yolo2_eval_coco_collect_workspace_bytes', 0, N, C) == 0
    one = ctypes.addressof(ctypes.create_string_buffer(4096))                          # never dereferenced: the checks fail first
    areas, ious = (ctypes.c_float * 8)(0, 1e10), (ctypes.c_float * 10)(*[0.5] * 10)
    good = [one] * 9 + [0, 1, 10, 20, 1, 0, 1, 0.1, ctypes.addressof(areas), 1, ctypes.addressof(ious), 10, 100, one, 16, one, one, one, 1 << 30, None]
    for at, bad in ((0, None), (8, None), (17, None), (19, None), (18, 0), (18, 5), (20, 11), (21, 0), (21, 129), (12, 1025), (13, 2), (15, 2), (23, 0)):
        args = list(good)
        args[at] = bad
        with pytest.raises(_lib.HipKernelError, match='argument check failed'):
            _lib.call('yolo2_eval_coco_collect', *args)
    ious[3] = float('nan')
    with pytest.raises(_lib.HipKernelError, match='argument check failed'):
        _lib.call('yolo2_eval_coco_collect', *good)
    slices, rec = (ctypes.c_int * 4)(0, 1, 0, 100), (ctypes.c_double * 3)(0.0, 0.5, 1.0)
    fgood = [one, 16, one, one, 20, 1, 10, 1, 10, 100, ctypes.addressof(slices), 2, ctypes.addressof(rec), 3, one, 1 << 30, one, None]
    for at, bad in ((0, None), (10, None), (12, None), (16, None), (11, 0), (11, 9), (13, 0), (13, 102), (15, 16), (9, 99), (7, 0)):
        args = list(fgood)
        args[at] = bad
        with pytest.raises(_lib.HipKernelError, match='argument check failed'):
            _lib.call('yolo2_eval_coco_finalize', *args)
    rec[1] = 2.0                                            # not ascending
    with pytest.raises(_lib.HipKernelError, match='argument check failed'):
        _lib.call('yolo2_eval_coco_finalize', *fgood)
