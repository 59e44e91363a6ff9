"""The on-device COCO evaluator on the MI355X against the NumPy checker (tests/coco_ref.py).  Records and npig are integers or bit
patterns and must be EQUAL; ap, recall and the twelve stats may differ by 1e-12 (sums of at most 101 f64 terms of at most 1, means of
at most a few hundred such values), with -1 in the same places."""
import os
import tempfile

import numpy as np
import pytest
import torch

import coco_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
SCALE = 32.0                                              # source pixels per cell of the synthetic cases (416 / 13)


def make_case(B, N, C, seed, density=0.02, grid=13.0, many=None, crowded=None):
    """Random sparse scores on a coarse grid of values (ties are common), boxes and ground truth in cell units, plus the planted traps
    of the rules.  many = (image, class, count): that many detections of one class in one image.  crowded = (boxes, of_one_class): one
    image with that many random ground truth boxes (the 9 planted ones come on top), of_one_class of them of class 0."""
    rng = np.random.RandomState(seed)
    lo = rng.uniform(0, grid - 2, (B, N, 2))
    boxes = np.concatenate([lo, lo + rng.uniform(0.2, 4, (B, N, 2))], -1).astype(np.float32)
    conf = ((rng.randint(1, 33, (B, N, C)) / 32.0) * (rng.uniform(size=(B, N, C)) < density)).astype(np.float32)
    scale = np.full((B, 2), SCALE, np.float32)
    scale[:, 1] = SCALE * (1 + 0.25 * (np.arange(B) % 3))                    # not square
    gt_class, gt_box, gt_flags, gt_area, first = [], [], [], [], [0]

    def add_gt(c, bx, flags=0, area=None):
        gt_class.append(c); gt_box.append(np.asarray(bx, np.float32)); gt_flags.append(flags)
        gt_area.append(None if area is None else np.float32(area))
    for b in range(B):
        k = 0 if b % 5 == 3 else int(rng.randint(1, 7))   # some images have no ground truth
        if crowded is not None:
            k = crowded[0]
        for j in range(k):
            c = int(rng.randint(0, C - 1)) if C > 1 else 0                   # the last class never has ground truth
            if crowded is not None:
                c = 0 if j < crowded[1] else int(rng.randint(1, max(C - 1, 2)))
            i = int(rng.randint(0, N))
            bx = boxes[b, i].copy()                       # a ground truth box that some detection box equals exactly
            if rng.uniform() < 0.5:
                bx[2:] += np.float32(rng.uniform(0, 1.5))
            u = rng.uniform()
            add_gt(c, bx, flags=1 if u < 0.15 else 2 if u < 0.2 else 3 if u < 0.22 else 0)
            for j2 in rng.randint(0, N, 3):               # several detections on one box, some with identical boxes and scores
                boxes[b, j2] = boxes[b, i] if rng.uniform() < 0.5 else boxes[b, i] + np.float32(rng.uniform(-0.3, 0.3))
                conf[b, j2, c] = conf[b, i, c] = np.float32(rng.randint(1, 33) / 32.0)
        if b % 4 == 0 and N >= 16 and C >= 3:
            for i in range(12):
                conf[b, i] = 0
            # (all planted boxes sit at x >= 100, away from the random ones, and score high enough to stay below max_dets)
            # box 0, class 0: IoU exactly .5 on integer coordinates: a match at t = .5 only
            add_gt(0, [101, 1, 102, 2])
            boxes[b, 0], conf[b, 0, 0] = [101, 1, 103, 2], 0.875
            # box 1, class 1: an ignored box at 80/100, one that counts at 60/100: the one that counts is matched
            add_gt(1, [104, 4, 114, 12], flags=1)
            add_gt(1, [104, 4, 110, 14])
            boxes[b, 1], conf[b, 1, 1] = [104, 4, 114, 14], 1.0
            # boxes 2, 3, class 2: equal overlaps (the later box wins), then a detection that equals the earlier box
            add_gt(2, [100, 20, 110, 28])
            add_gt(2, [100, 22, 110, 30])
            boxes[b, 2], conf[b, 2, 2] = [100, 20, 110, 30], 1.0
            boxes[b, 3], conf[b, 3, 2] = [100, 20, 110, 28], 0.96875
            # boxes 4-6, class 0: inside a crowd box
            add_gt(0, [120, 20, 130, 30], flags=2)
            for i, s in ((4, 1.0), (5, 1.0), (6, 0.96875)):
                boxes[b, i], conf[b, i, 0] = [121 + i - 4, 21, 123 + i - 4, 24], s
            # boxes 7, 8, class 1: the second detection falls through to the next best free box
            add_gt(1, [140, 0, 150, 10])
            add_gt(1, [140, 0, 150, 7])
            boxes[b, 7], conf[b, 7, 1] = [140, 0, 150, 10], 0.9375
            boxes[b, 8], conf[b, 8, 1] = [140, 0, 150, 9], 0.9375            # (equal scores: the box index decides)
            # box 9, class 2: unmatched, about 20 x 20 source pixels: a false positive in "all" and "small", ignored in the others
            boxes[b, 9], conf[b, 9, 2] = [160, 60, 160 + 20 / scale[b, 0], 60 + 20 / scale[b, 1]], 0.9375
            # a ground truth box with an area of its own (a segmentation's): large by its box, small by its area
            add_gt(0, [170, 70, 180, 80], area=500.0)
            boxes[b, 10], conf[b, 10, 0] = [170, 70, 180, 80], 0.90625
        first.append(len(gt_class))
        if b % 7 == 5:
            conf[b] = 0                                    # an image without any detection
    if many is not None:
        b, c, n = many
        conf[b, :n] = 0
        conf[b, :n, c] = (rng.randint(1, 33, n) / 32.0).astype(np.float32)
    gt_box = np.asarray(gt_box, np.float32).reshape(-1, 4)
    img = np.repeat(np.arange(B), np.diff(first))
    area = np.array([((bx[2] - bx[0]) * scale[i, 0]) * ((bx[3] - bx[1]) * scale[i, 1]) if a is None else a for bx, a, i in zip(gt_box, gt_area, img)],
                    np.float32)
    return dict(conf=conf, xy_min=np.ascontiguousarray(boxes[..., :2]), xy_max=np.ascontiguousarray(boxes[..., 2:]),
                gt_class=np.asarray(gt_class, np.int32), gt_box=gt_box, gt_area=area, gt_flags=np.asarray(gt_flags, np.uint8),
                gt_first=np.asarray(first, np.int32), scale=scale)


GT_KEYS = ('gt_class', 'gt_box', 'gt_area', 'gt_flags', 'gt_first', 'scale')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def add_case(ev, case, image_base=0, n_valid=None):
    from yolo_tf_amd import evaluate
    gt = evaluate.device_gt_coco(*[case[k] for k in GT_KEYS])
    t = [dev(case[k]) for k in ('conf', 'xy_min', 'xy_max')]
    ev.add(*t, *gt, image_base=image_base, n_valid=n_valid)
    return t, gt


def ref_collect(case, mode, threshold, image_base=0, n_valid=None, **kw):
    B = case['conf'].shape[0]
    return coco_ref.collect(case['conf'], case['xy_min'], case['xy_max'], *[case[k] for k in GT_KEYS], image_base,
                            B if n_valid is None else n_valid, threshold, mode, **kw)


def rows(got):
    """Device records -> tuples of (image, class, rank, box, score bits, matched bits, ignored bits)."""
    return list(zip(got['image'].tolist(), got['class'].tolist(), got['rank'].tolist(), got['box'].tolist(), got['score'].view(np.uint32).tolist(),
                    got['matched'].tolist(), got['ignored'].tolist()))


def ref_rows(want):
    return [(r['image'], r['cls'], r['rank'], r['box'], int(np.float32(r['score']).view(np.uint32)), coco_ref.bits(r['matched']),
             coco_ref.bits(r['ignored'])) for r in want]


def assert_records_equal(got, want):
    g, w = rows(got), ref_rows(want)
    assert len(g) == len(w), (len(g), len(w))
    assert sorted(g) == sorted(w)                          # as sets ...
    assert g == w                                          # ... and in emitted order, bit for bit
    assert not got['reserved'].any()


def assert_result_equal(res, ref):
    assert res['detections'] == ref['detections']
    np.testing.assert_array_equal(res['npig'], ref['npig'])
    for k in ('ap', 'recall'):
        np.testing.assert_array_equal(res[k] == -1, ref[k] == -1)
        assert np.abs(res[k] - ref[k]).max(initial=0.0) <= TOL, k
    if 'stats' in ref:
        assert len(res['stats']) == 12
        for a, b in zip(res['stats'], ref['stats']):
            assert (a == -1) == (b == -1) and abs(a - b) <= TOL, (res['stats'], ref['stats'])


def assert_traps(case, want):
    """The planted situations really occur in the checker's output (image 0 carries them)."""
    at = {(r['image'], r['box'], r['cls']): r for r in want}
    r = at[(0, 0, 0)]
    assert r['matched'][0, 0] and not r['matched'][0, 1]                                # IoU == .5 matches at t = .5 only
    r = at[(0, 1, 1)]
    assert r['matched'][0, 0] and not r['ignored'][0, 0] and r['matched'][0, 4] and r['ignored'][0, 4]      # the break rule
    assert at[(0, 2, 2)]['matched'][0, 5] and at[(0, 3, 2)]['matched'][0, 9]            # equal overlaps: the later box was taken
    assert all(at[(0, i, 0)]['matched'].all() and at[(0, i, 0)]['ignored'].all() for i in (4, 5, 6))      # crowd
    assert at[(0, 7, 1)]['rank'] < at[(0, 8, 1)]['rank'] and at[(0, 8, 1)]['matched'][0, 5] and not at[(0, 8, 1)]['matched'][0, 6]
    r = at[(0, 9, 2)]
    assert not r['matched'].any() and r['ignored'][:, 0].tolist() == [False, False, True, True]
    r = at[(0, 10, 0)]
    assert r['matched'][1, 0] and not r['ignored'][1, 0] and r['ignored'][3, 0]         # small by its own area
    keys = [(r['image'], r['cls'], int(np.float32(r['score']).view(np.uint32))) for r in want]
    assert len(set(keys)) < len(keys)                                                   # tied scores inside an (image, class)


# B, N, C, density, extras
SHAPES = {'small': (3, 98, 20, 0.05, {}),
          'general': (8, 845, 20, 0.02, {}),
          'coco80': (2, 1805, 80, 0.005, dict(many=(1, 7, 150))),
          'crowded': (1, 256, 3, 0.3, dict(crowded=(503, 200), grid=40.0)),
          'sort': (64, 845, 20, 0.02, dict(detect_density=0.03))}     # (one detection per box: 0.02 stays below 16384 records in mode detect)
_cache = {}


def reference(name, mode):
    """(case, the checker's records, npig, result) of a shape: computed once, shared, never modified."""
    if (name, mode) not in _cache:
        B, N, C, density, extra = SHAPES[name]
        extra = dict(extra)
        detect_density = extra.pop('detect_density', density)
        density = detect_density if mode == 'detect' else density
        case = make_case(B, N, C, seed=B * 1000 + N + C, density=density, **extra)
        want, npig = ref_collect(case, mode, 0.1)
        _cache[(name, mode)] = (case, want, npig, coco_ref.evaluate(want, npig, C))
    return _cache[(name, mode)]


@pytest.mark.parametrize('mode', ['detect', 'all'])
@pytest.mark.parametrize('name', sorted(SHAPES))
def test_collect_and_finalize_equal_the_checker(name, mode):
    from yolo_tf_amd.evaluate import CocoEvaluator
    C = SHAPES[name][2]
    case, want, npig, ref = reference(name, mode)
    assert_traps(case, want)
    if name == 'coco80':                                   # the planted class is cut at max_dets
        n = int(((case['conf'][1].argmax(1) == 7) & (case['conf'][1].max(1) > 0.1)).sum()) if mode == 'detect' else int((case['conf'][1, :, 7] > 0.1).sum())
        assert n >= 140 and max(r['rank'] for r in want if r['image'] == 1 and r['cls'] == 7) == 99
    if name == 'crowded':                                  # exactly the per-image limit
        assert len(case['gt_class']) == 512 and int((case['gt_class'] == 0).sum()) >= 200
    if name == 'sort':
        assert len(want) > 16384                           # more than one tile of the radix passes
    if C > 3:
        assert npig[0, C - 1] == 0 and (ref['ap'][:, :, C - 1] == -1).all()  # the class without ground truth
    ev = CocoEvaluator(C, max(len(want), 1), mode=mode, threshold=0.1)
    add_case(ev, case)
    assert_records_equal(ev.records_numpy(), want)
    np.testing.assert_array_equal(ev.npig.cpu().numpy().reshape(npig.shape), npig)
    assert_result_equal(ev.result(), ref)


def split(case, lo, hi, pad_to=None):
    """Images lo..hi-1 of a case as a batch of its own; padded to pad_to images with image 0 INCLUDING its ground truth and scores."""
    idx = list(range(lo, hi)) + [0] * ((pad_to or (hi - lo)) - (hi - lo))
    first = [0]
    parts = {k: [] for k in ('gt_class', 'gt_box', 'gt_area', 'gt_flags')}
    for i in idx:
        a, b = case['gt_first'][i], case['gt_first'][i + 1]
        for k in parts:
            parts[k].append(case[k][a:b])
        first.append(first[-1] + (b - a))
    out = {k: np.concatenate(v) for k, v in parts.items()}
    out.update(conf=case['conf'][idx], xy_min=case['xy_min'][idx], xy_max=case['xy_max'][idx], scale=case['scale'][idx], gt_first=np.asarray(first, np.int32))
    return out


def result_bits(res):
    return (res['ap'].tobytes(), res['recall'].tobytes(), res['npig'].tobytes(), np.asarray(res['stats']).tobytes(), res['detections'])


def test_accumulation_over_three_calls_with_a_padded_last_batch_equals_one_call():
    from yolo_tf_amd.evaluate import CocoEvaluator
    case, want, npig, ref = reference('general', 'all')
    assert case['gt_first'][1] > 0 and (case['conf'][0] > 0.1).any()        # the padding image owns ground truth and detections
    outs = []
    for sizes, B in (([8], 8), ([3, 3, 2], 3)):
        ev = CocoEvaluator(20, len(want), mode='all', threshold=0.1)
        base, keep = 0, []
        for n in sizes:
            keep.append(add_case(ev, split(case, base, base + n, pad_to=B), image_base=base, n_valid=n))
            base += n
        outs.append((ev.records_numpy().tobytes(), result_bits(ev.result())))
    assert outs[0] == outs[1] and outs[0][1][-1] == len(want)


def test_two_runs_are_bitwise_equal():
    from yolo_tf_amd.evaluate import CocoEvaluator
    case, want, _, _ = reference('sort', 'all')
    outs = []
    for _ in range(2):
        ev = CocoEvaluator(20, 2 * len(want), mode='all', threshold=0.1)
        add_case(ev, case)
        add_case(ev, case, image_base=64)
        outs.append((ev.records_numpy().tobytes(), result_bits(ev.result())))
    assert outs[0] == outs[1] and outs[0][1][-1] == 2 * len(want)
    ev.reset()
    assert ev.result()['detections'] == 0


def test_a_buffer_one_record_too_small_raises_and_nothing_is_written_behind_it():
    from yolo_tf_amd._lib import HipKernelError
    from yolo_tf_amd.evaluate import CocoEvaluator
    case, want, _, _ = reference('general', 'all')
    need = len(want)
    ev = CocoEvaluator(20, need - 1, mode='all', threshold=0.1)
    guard = 1 << 16
    big = torch.full((40 * (need - 1) + guard,), 0xAB, dtype=torch.uint8, device='cuda')
    ev.records = big[:40 * (need - 1)]
    add_case(ev, case)
    add_case(ev, case, image_base=8)                      # a whole batch behind the end
    with pytest.raises(HipKernelError, match=r'\b%d are needed' % (2 * need)):
        ev.result()
    assert bool((big[40 * (need - 1):] == 0xAB).all())
    assert_records_equal(big[:40 * (need - 1)].cpu().numpy().view(ev.records_numpy().dtype), want[:need - 1])


def test_custom_tables():
    """One threshold, one area range, at most 10 detections per (image, class)."""
    from yolo_tf_amd.evaluate import CocoEvaluator
    case = reference('coco80', 'all')[0]
    ranges, thr, slices = np.array([[0, 1e10]], np.float32), np.array([0.5], np.float32), [(0, 1), (0, 10)]
    want, npig = ref_collect(case, 'all', 0.1, area_ranges=ranges, iou_thresholds=thr, max_dets=10)
    assert max(r['rank'] for r in want) == 9
    ap, recall = coco_ref.accumulate(want, npig, 80, slices=slices, n_iou=1)
    ev = CocoEvaluator(80, len(want), mode='all', threshold=0.1, iou_thresholds=thr, area_ranges=ranges, max_dets=10)
    assert ev.slices.tolist() == [list(s) for s in slices]
    add_case(ev, case)
    assert_records_equal(ev.records_numpy(), want)
    res = ev.result()
    assert res['ap'].shape == (2, 1, 80) and res['npig'].shape == (1, 80)
    assert_result_equal(res, dict(ap=ap, recall=recall, npig=npig, detections=len(want)))
    s = res['stats']
    assert s[0] == s[1] and abs(s[0] - coco_ref._mean(ap[1])) <= TOL and s[2] == -1 and s[3:6] == [-1] * 3 and s[8:] == [-1] * 4
    assert abs(s[6] - coco_ref._mean(recall[0])) <= TOL and abs(s[7] - coco_ref._mean(recall[1])) <= TOL


def test_argument_errors_raise_without_a_launch():
    from yolo_tf_amd import ops
    from yolo_tf_amd._lib import HipKernelError
    from yolo_tf_amd.evaluate import CocoEvaluator
    case = reference('small', 'all')[0]
    new = lambda **kw: CocoEvaluator(20, 4096, mode='all', threshold=0.1, **kw)
    for kw in (dict(iou_thresholds=np.linspace(.5, .95, 11)), dict(iou_thresholds=[0.5, float('nan')]), dict(area_ranges=np.zeros((5, 2))),
               dict(area_ranges=[[0, float('nan')]]), dict(max_dets=129), dict(max_dets=0, slices=[(0, 1)])):
        with pytest.raises(HipKernelError, match='argument check failed'):
            add_case(new(**kw), case)
    for kw in (dict(recall_thresholds=np.linspace(0, 1, 102)), dict(recall_thresholds=[0.0, float('nan')]), dict(recall_thresholds=[0.5, 0.25]),
               dict(slices=[(4, 1)]), dict(slices=[(0, 101)]), dict(slices=[(0, 1)] * 9)):
        ev = new(**kw)
        add_case(ev, case)
        with pytest.raises(HipKernelError, match='argument check failed'):
            ev.result()
    ev = new()
    with pytest.raises(HipKernelError, match='argument check failed'):      # null pointers
        ops.eval_coco_collect(None, None, None, None, None, None, None, None, None, 0, 1, 98, 20, 1, 0, 1, 0.1, ev.area_ranges, 4, ev.iou_thresholds, 10,
                              100, ev.records, 4096, ev.state, ev.npig, None)
    with pytest.raises(HipKernelError, match='argument check failed'):
        ops.eval_coco_finalize(ev.records, 4096, ev.state, ev.npig, 20, 1, 98, 4, 10, 100, None, 6, None, 101, None, ev.results)
    assert int(ev.state[0].item()) == 0                    # nothing ran
    with pytest.raises(HipKernelError, match='argument check failed'):      # more classes than the per-image class table holds
        add_case(CocoEvaluator(1025, 16, mode='all'), dict(case, conf=np.zeros((3, 98, 1025), np.float32)))


def make_builder(size, basedir):
    from yolo_tf_amd import utils
    from yolo_tf_amd.model import yolo2
    cfg = utils.make_config([os.path.join(ROOT, 'config.ini'), os.path.join(ROOT, 'config', 'yolo2', 'tiny-20.ini')], basedir)
    cfg.set('cache', 'names', os.path.join(ROOT, cfg.get('cache', 'names')))
    cfg.set('yolo2', 'anchors', os.path.join(ROOT, cfg.get('yolo2', 'anchors')))
    cfg.set('yolo2', 'width', str(size))
    cfg.set('yolo2', 'height', str(size))
    utils.ensure_names(cfg)
    b = yolo2.Builder(None, cfg)
    b(None)
    return b


class FiniteBoxes(object):
    """A DetectSession whose detect() replaces non-finite box coordinates: random weights overflow the decoder's exp(), and overlaps
    of NaN boxes are outside the rules (Python's min / max in the checker and the device's fminf / fmaxf treat NaN differently)."""

    def __init__(self, session):
        self.session = session

    def __getattr__(self, name):
        return getattr(self.session, name)

    def detect(self, *args, **kw):
        out = self.session.detect(*args, **kw)
        for t in (self.session.xy_min, self.session.xy_max):
            torch.nan_to_num_(t, nan=0.0, posinf=1e4, neginf=-1e4)
        return out


def test_end_to_end_through_evaldata_and_a_detect_session():
    """Tiny YOLO VOC-20 with random weights, batch 4, 10 synthetic images of mixed sizes (4 + 4 + 2 padded): every batch's device
    buffers are downloaded and scored by the checker, which isolates the evaluator from the network's numerics."""
    from yolo_tf_amd import evaluate
    from yolo_tf_amd.session import DetectSession
    with tempfile.TemporaryDirectory() as basedir:
        builder = make_builder(224, basedir)
        sess = FiniteBoxes(DetectSession(builder, 4, dtype='bf16', seed=4))
        m = sess.model
        images, objects, difficult = evaluate.synthetic_dataset(10, 20, seed=9)
        crowd = [(np.arange(len(d)) % 3 == 2).astype(np.uint8) for d in difficult]
        assert sum(int(d.sum()) for d in difficult) > 0 and sum(int(c.sum()) for c in crowd) > 0
        data = evaluate.EvalData(images, objects, 4, builder.width, builder.height, m.cell_width, m.cell_height, difficult=difficult, crowd=crowd)
        want, npig = [], np.zeros((4, 20), np.int64)

        def on_batch(s, gt, base, n_valid):
            r, n = coco_ref.collect(s.conf.cpu().numpy(), s.xy_min.cpu().numpy(), s.xy_max.cpu().numpy(), *data.batch_gt_coco(base, n_valid), base, n_valid,
                                    0.01, 'all')
            want.extend(r)
            npig[:] += n
        ev = evaluate.CocoEvaluator(20, 10 * 100 * 20, mode='all', threshold=0.01)
        res = evaluate.evaluate(builder, sess, data, mode='all', threshold=0.01, threshold_iou=0.45, evaluator=ev, on_batch=on_batch, protocol='coco')
        assert len(want) > 100 and res['detections'] == len(want)           # the threshold is low enough for random weights
        flags = np.concatenate(data.flags)
        assert int(npig[0].sum()) == int((flags == 0).sum()) and set(flags.tolist()) >= {0, 1, 2}
        assert_records_equal(ev.records_numpy(), want)
        assert_result_equal(res, coco_ref.evaluate(want, npig, 20))
