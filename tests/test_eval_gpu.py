"""The on-device evaluator on the MI355X against the NumPy checker (tests/eval_ref.py).  Everything compared is an integer or a bit
pattern and must be EQUAL; only the two f64 average precisions may differ, by at most 1e-9: sums of at most about 1e7 f64 terms of
magnitude at most 1 in a different association differ by far less (1e7 * 2^-53 ~ 1e-9 is already a crude upper bound)."""
import os
import tempfile

import numpy as np
import pytest
import torch

import eval_ref
from eval_ref import FP, IGNORED, TP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AP_TOL = 1e-9


def make_case(B, N, C, seed, density=0.02, grid=13.0):
    """Random sparse scores, boxes and ground truth in cell units, plus the planted traps of the rules."""
    rng = np.random.RandomState(seed)
    lo = rng.uniform(0, grid - 2, (B, N, 2))
    boxes = np.concatenate([lo, lo + rng.uniform(0.5, 4, (B, N, 2))], -1).astype(np.float32)
    # scores on a coarse grid of values: duplicates within and across images are the rule, not the exception
    conf = (rng.randint(1, 33, (B, N, C)) / 32.0).astype(np.float32) * (rng.uniform(size=(B, N, C)) < density)
    conf = conf.astype(np.float32)
    gt_class, gt_box, gt_dif, first = [], [], [], [0]
    hard_class = C - 1                                    # every ground truth box of this class is difficult
    for b in range(B):
        k = 0 if b % 5 == 3 else int(rng.randint(1, 7))   # some images have no ground truth
        for _ in range(k):
            c = int(rng.randint(0, C))
            i = int(rng.randint(0, N))
            bx = boxes[b, i].copy()                       # a ground truth box that some detection box equals exactly
            if rng.uniform() < 0.5:
                bx[2:] += np.float32(rng.uniform(0, 1.5))
            gt_class.append(c)
            gt_box.append(bx)
            gt_dif.append(1 if c == hard_class else int(rng.uniform() < 0.2))
            for j in rng.randint(0, N, 3):                # several detections on one ground truth box, some with identical boxes and scores
                boxes[b, j] = boxes[b, i] if rng.uniform() < 0.5 else boxes[b, i] + np.float32(rng.uniform(-0.3, 0.3))
                conf[b, j, c] = conf[b, i, c] = np.float32(rng.randint(1, 33) / 32.0)
        if b % 4 == 0 and N >= 8:
            # IoU exactly at the threshold 0.5 on integer coordinates: not a match
            c = 0
            gt_class.append(c); gt_box.append(np.array([1, 1, 2, 2], np.float32)); gt_dif.append(0)
            boxes[b, 0] = [1, 1, 3, 2]
            conf[b, 0] = 0
            conf[b, 0, c] = 0.75
            # best candidate difficult (IoU 0.8) while a non-difficult one overlaps less (IoU 0.6): ignored, and the other stays unmatched
            c = 1 % C
            gt_class.append(c); gt_box.append(np.array([4, 4, 14, 12], np.float32)); gt_dif.append(1)
            gt_class.append(c); gt_box.append(np.array([4, 4, 10, 14], np.float32)); gt_dif.append(0)
            boxes[b, 1] = [4, 4, 14, 14]
            conf[b, 1] = 0
            conf[b, 1, c] = 0.875
            k += 3
        first.append(len(gt_class))
        if b % 7 == 5:
            conf[b] = 0                                    # an image without any detection
    return dict(conf=conf, xy_min=np.ascontiguousarray(boxes[..., :2]), xy_max=np.ascontiguousarray(boxes[..., 2:]),
                gt_class=np.asarray(gt_class, np.int32), gt_box=np.asarray(gt_box, np.float32).reshape(-1, 4),
                gt_difficult=np.asarray(gt_dif, np.uint8), gt_first=np.asarray(first, np.int32))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def add_case(ev, case, image_base=0, n_valid=None):
    from yolo_tf_amd import evaluate
    gt = evaluate.device_gt(case['gt_class'], case['gt_box'], case['gt_difficult'], case['gt_first'])
    t = [dev(case[k]) for k in ('conf', 'xy_min', 'xy_max')]
    ev.add(*t, *gt, image_base=image_base, n_valid=n_valid)
    return t, gt


def ref_collect(case, mode, threshold, iou, image_base=0, n_valid=None):
    B = case['conf'].shape[0]
    return eval_ref.collect(case['conf'], case['xy_min'], case['xy_max'], case['gt_class'], case['gt_box'], case['gt_difficult'], case['gt_first'],
                            image_base, B if n_valid is None else n_valid, threshold, iou, mode)


def assert_records_equal(got, want):
    """got: structured array of yolo2_eval_record; want: the checker's list of (score, class, flag, image, box) in emitted order."""
    s, c, f, i, b = eval_ref.as_arrays(want)
    assert len(got) == len(s), (len(got), len(s))
    # as sets per (image, class) ...
    key = lambda cls, img, box, sc, fl: sorted(zip(img.tolist(), cls.tolist(), box.tolist(), sc.view(np.uint32).tolist(), fl.tolist()))
    gc, gf = (got['class_flag'] >> 2).astype(np.int64), (got['class_flag'] & 3).astype(np.int64)
    assert key(gc, got['image'], got['box'], got['score'], gf) == key(c, i, b, s, f)
    # ... and in emitted order, bit for bit
    np.testing.assert_array_equal(got['score'].view(np.uint32), s.view(np.uint32))
    np.testing.assert_array_equal(gc, c)
    np.testing.assert_array_equal(gf, f)
    np.testing.assert_array_equal(got['image'], i)
    np.testing.assert_array_equal(got['box'], b)


def assert_result_equal(ev, res, ref, C):
    """Evaluator.result() + curve() against eval_ref.evaluate()."""
    for k in ('npos', 'tp', 'fp', 'ignored', 'detections'):
        assert res[k] == ref[k], k
    for k in ('ap07', 'ap12'):
        got, want = np.asarray(res[k]), np.asarray(ref[k])
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.abs(got[ok] - want[ok]).max(initial=0.0) <= AP_TOL, (k, got, want)
    for k in ('mAP07', 'mAP12'):
        assert (np.isnan(res[k]) and np.isnan(ref[k])) or abs(res[k] - ref[k]) <= AP_TOL
    recs, ctp, cfp = ev.curve()
    cls, flag = recs['class_flag'] >> 2, recs['class_flag'] & 3
    live = flag != IGNORED
    assert not live[int(live.sum()):].any()               # the ignored records sort behind all others
    start = 0
    for c in range(C):
        n = len(ref['order'][c])
        seg = slice(start, start + n)
        assert (cls[seg] == c).all() and live[seg].all()
        np.testing.assert_array_equal(np.stack([recs['image'][seg], recs['box'][seg]], 1), ref['order'][c])
        np.testing.assert_array_equal(ctp[seg], ref['cum_tp'][c])
        np.testing.assert_array_equal(cfp[seg], ref['cum_fp'][c])
        start += n
    assert start == int(live.sum())


SHAPES = [(1, 845, 20, 0.02), (8, 845, 20, 0.02), (4, 1805, 80, 0.005), (3, 98, 20, 0.05), (256, 845, 20, 0.002)]


@pytest.mark.parametrize('mode', ['detect', 'all'])
@pytest.mark.parametrize('B,N,C,density', SHAPES)
def test_collect_and_finalize_equal_the_checker(B, N, C, density, mode):
    from yolo_tf_amd.evaluate import Evaluator
    case = make_case(B, N, C, seed=B * 1000 + N + C, density=density)
    want, npos = ref_collect(case, mode, 0.1, 0.5)
    flags = [r[2] for r in want]
    if B >= 4:        # the traps are really there
        assert TP in flags and FP in flags and IGNORED in flags
    ev = Evaluator(C, max(len(want), 1), mode=mode, threshold=0.1, iou_threshold=0.5, keep_curve=True)
    add_case(ev, case)
    assert_records_equal(ev.records_numpy(), want)
    np.testing.assert_array_equal(ev.npos.cpu().numpy(), npos)
    assert npos[C - 1] == 0                               # the all-difficult class
    assert_result_equal(ev, ev.result(), eval_ref.evaluate(want, npos, C), C)


def test_worked_example_on_the_device():
    from yolo_tf_amd.evaluate import Evaluator
    boxes = np.zeros((2, 3, 4), np.float32)
    conf = np.zeros((2, 3, 1), np.float32)
    boxes[0, 0], conf[0, 0] = [0, 0, 10, 8], 0.9
    boxes[0, 1], conf[0, 1] = [0, 0, 10, 6], 0.8
    boxes[0, 2], conf[0, 2] = [20, 0, 30, 7], 0.7
    boxes[1, 0], conf[1, 0] = [0, 0, 10, 3], 0.6
    boxes[1, 1], conf[1, 1] = [0, 0, 10, 9], 0.5
    case = dict(conf=conf, xy_min=np.ascontiguousarray(boxes[..., :2]), xy_max=np.ascontiguousarray(boxes[..., 2:]), gt_class=np.zeros(3, np.int32),
                gt_box=np.array([[0, 0, 10, 10], [20, 0, 30, 10], [0, 0, 10, 10]], np.float32), gt_difficult=np.array([0, 1, 0], np.uint8),
                gt_first=np.array([0, 2, 3], np.int32))
    for mode in ('detect', 'all'):
        ev = Evaluator(1, 16, mode=mode, threshold=0.1, iou_threshold=0.5)
        add_case(ev, case)
        r = ev.result()
        assert (ev.records_numpy()['class_flag'] & 3).tolist() == [TP, FP, IGNORED, FP, TP]
        assert r['npos'] == [2] and r['tp'] == [2] and r['fp'] == [2] and r['ignored'] == [1] and r['detections'] == 5
        assert abs(r['ap12'][0] - 0.75) <= AP_TOL and abs(r['ap07'][0] - 8.5 / 11) <= AP_TOL
        assert isinstance(r['mAP07'], float) and isinstance(r['mAP12'], float)


def test_sort_of_more_than_a_million_records():
    """Stage B alone on synthetic records: the sort spans 74 tiles of 16384 records; scores are heavily tied."""
    from yolo_tf_amd.evaluate import Evaluator, RECORD_DTYPE
    rng = np.random.RandomState(5)
    M, C, I, N = 1200000, 20, 4952, 845
    where = rng.permutation(I * N)[:M]                    # distinct (image, box): the order is total
    recs = np.zeros(M, RECORD_DTYPE)
    recs['score'] = (rng.randint(1, 4097, M) / 4096.0).astype(np.float32)
    recs['image'], recs['box'] = where // N, where % N
    cls = rng.randint(0, C, M)
    cls[cls == 7] = 8                                     # a class without records
    flag = rng.choice([FP, TP, IGNORED], M, p=[0.7, 0.25, 0.05])
    recs['class_flag'] = (cls << 2 | flag).astype(np.uint32)
    npos = np.array([int(((cls == c) & (flag == TP)).sum()) + int(rng.randint(0, 1000)) for c in range(C)], np.int32)
    npos[3], npos[7] = 0, 5                               # NaN although it has records; 0 because it has none
    ev = Evaluator(C, M + 1000, mode='all', keep_curve=True)
    ev.records[:16 * M] = torch.from_numpy(recs.view(np.uint8)).cuda()
    ev.state[0] = M
    ev.npos.copy_(torch.from_numpy(npos).cuda())
    ev.n_images, ev.N = I, N
    res = ev.result()
    ref = eval_ref.evaluate((recs['score'], cls.astype(np.int64), flag.astype(np.int64), recs['image'].astype(np.int64), recs['box'].astype(np.int64)), npos, C)
    assert_result_equal(ev, res, ref, C)
    assert np.isnan(res['ap07'][3]) and res['ap07'][7] == 0.0 and res['detections'] == M
    res2 = ev.result()                                    # finalize reads the records, it does not consume them
    assert np.array_equal(np.asarray(res['ap12']).view(np.uint64), np.asarray(res2['ap12']).view(np.uint64))


def split(case, lo, hi, pad_to=None):
    """Images lo..hi-1 of a case as a batch of its own; padded to pad_to images with image 0 INCLUDING its ground truth and scores."""
    idx = list(range(lo, hi)) + [0] * ((pad_to or (hi - lo)) - (hi - lo))
    first = [0]
    gc, gb, gd = [], [], []
    for i in idx:
        a, b = case['gt_first'][i], case['gt_first'][i + 1]
        gc.append(case['gt_class'][a:b]); gb.append(case['gt_box'][a:b]); gd.append(case['gt_difficult'][a:b])
        first.append(first[-1] + (b - a))
    return dict(conf=case['conf'][idx], xy_min=case['xy_min'][idx], xy_max=case['xy_max'][idx], gt_class=np.concatenate(gc), gt_box=np.concatenate(gb),
                gt_difficult=np.concatenate(gd), gt_first=np.asarray(first, np.int32))


def bits(res):
    return [np.asarray(res[k], np.float64).view(np.uint64).tolist() for k in ('ap07', 'ap12', 'mAP07', 'mAP12')] + \
           [res[k] for k in ('npos', 'tp', 'fp', 'ignored', 'detections')]


@pytest.mark.parametrize('mode', ['detect', 'all'])
def test_accumulation_and_padding(mode):
    from yolo_tf_amd.evaluate import Evaluator
    case = make_case(24, 845, 20, seed=11, density=0.01)
    cap = len(ref_collect(case, mode, 0.1, 0.5)[0])
    assert case['gt_first'][1] > 0 and (case['conf'][0] > 0.1).any()        # the padding image owns ground truth and detections
    outs = []
    for sizes, B in (([24], 24), ([8, 8, 8], 8), ([5, 5, 5, 5, 4], 5)):
        ev = Evaluator(20, cap, mode=mode, threshold=0.1, iou_threshold=0.5)
        base, keep = 0, []
        for n in sizes:
            keep.append(add_case(ev, split(case, base, base + n, pad_to=B), image_base=base, n_valid=n))
            base += n
        outs.append((ev.records_numpy().tobytes(), bits(ev.result())))
    assert outs[0][1][-1] == cap
    assert outs[0] == outs[1] and outs[0] == outs[2]


def test_two_runs_are_bitwise_equal():
    from yolo_tf_amd.evaluate import Evaluator
    case = make_case(64, 845, 20, seed=3, density=0.05)
    outs = []
    for _ in range(2):
        ev = Evaluator(20, 64 * 845 * 20, mode='all', threshold=0.1, iou_threshold=0.5, keep_curve=True)
        add_case(ev, case)
        add_case(ev, case, image_base=64)
        res = ev.result()
        outs.append((ev.records_numpy().tobytes(), bits(res), [a.tobytes() for a in ev.curve()]))
    assert outs[0] == outs[1] and outs[0][1][-1] > 50000
    ev.reset()
    assert ev.result()['detections'] == 0


def test_a_buffer_one_record_too_small_raises_and_nothing_is_written_behind_it():
    from yolo_tf_amd._lib import HipKernelError
    from yolo_tf_amd.evaluate import Evaluator
    case = make_case(8, 845, 20, seed=21, density=0.02)
    need = len(ref_collect(case, 'all', 0.1, 0.5)[0])
    ev = Evaluator(20, need - 1, mode='all', threshold=0.1, iou_threshold=0.5)
    guard = 1 << 16
    big = torch.full((16 * (need - 1) + guard,), 0xAB, dtype=torch.uint8, device='cuda')
    ev.records = big[:16 * (need - 1)]
    add_case(ev, case)
    add_case(ev, case, image_base=8)                      # a whole batch behind the end
    with pytest.raises(HipKernelError, match=r'\b%d are needed' % (2 * need)):
        ev.result()
    assert bool((big[16 * (need - 1):] == 0xAB).all())
    want, _ = ref_collect(case, 'all', 0.1, 0.5)
    assert_records_equal(big[:16 * (need - 1)].cpu().numpy().view(ev.records_numpy().dtype), want[:need - 1])
    ev2 = Evaluator(20, need, mode='all', threshold=0.1, iou_threshold=0.5)
    add_case(ev2, case)
    assert ev2.result()['detections'] == need


def make_builder(size, basedir):
    from yolo_tf_amd import utils
    from yolo_tf_amd.model import yolo2
    cfg = utils.make_config([os.path.join(ROOT, 'config.ini'), os.path.join(ROOT, 'config', 'yolo2', 'darknet-20.ini')], basedir)
    cfg.set('cache', 'names', os.path.join(ROOT, cfg.get('cache', 'names')))
    cfg.set('yolo2', 'anchors', os.path.join(ROOT, cfg.get('yolo2', 'anchors')))
    cfg.set('yolo2', 'width', str(size))
    cfg.set('yolo2', 'height', str(size))
    utils.ensure_names(cfg)
    b = yolo2.Builder(None, cfg)
    b(None)
    return b


@pytest.fixture(scope='module')
def basedir():
    with tempfile.TemporaryDirectory() as d:
        yield d


def test_planted_detections_in_a_detect_session(basedir):
    """Decoded boxes written straight into a DetectSession's buffers: equal to the ground truth -> mAP 1; every second one moved away
    -> the closed form below."""
    from yolo_tf_amd.evaluate import Evaluator, device_gt
    from yolo_tf_amd.session import DetectSession
    sess = DetectSession(make_builder(96, basedir), 8, dtype='f32')
    B, N, C = sess.B, sess.N, sess.C
    assert (N, C) == (45, 20)
    # image b: two ground truth boxes of class b % 4, planted at boxes 3 and 7
    gt_class = np.repeat(np.arange(B) % 4, 2).astype(np.int32)
    gt_box = np.tile(np.array([[0.25, 0.5, 1.5, 2.0], [1.0, 0.75, 2.75, 2.5]], np.float32), (B, 1))
    gt = device_gt(gt_class, gt_box, np.zeros(2 * B, np.uint8), np.arange(0, 2 * B + 1, 2).astype(np.int32))
    for shifted in (False, True):
        conf = np.zeros((B, N, C), np.float32)
        boxes = np.zeros((B, N, 4), np.float32)
        for b in range(B):
            boxes[b, 3], boxes[b, 7] = gt_box[2 * b], gt_box[2 * b + 1]
            conf[b, 3, b % 4], conf[b, 7, b % 4] = 1.0, 1.0
            if shifted:                                   # the second one: out of overlap, and behind every TP in the order
                boxes[b, 7] += 100.0
                conf[b, 7, b % 4] = 0.5
        sess.conf.copy_(dev(conf)); sess.xy_min.copy_(dev(boxes[..., :2])); sess.xy_max.copy_(dev(boxes[..., 2:]))
        for mode in ('detect', 'all'):
            ev = Evaluator(C, B * N * C, mode=mode, threshold=0.005, iou_threshold=0.5)
            ev.add(sess.conf, sess.xy_min, sess.xy_max, *gt, image_base=0)
            r = ev.result()
            assert r['npos'] == [4] * 4 + [0] * 16 and r['detections'] == 2 * B
            assert all(np.isnan(v) for v in r['ap07'][4:] + r['ap12'][4:])
            if not shifted:
                assert r['mAP07'] == 1.0 and r['mAP12'] == 1.0 and r['tp'][:4] == [4] * 4 and r['fp'] == [0] * C
            else:
                # per class: TP TP FP FP with 4 positives: recall .25 .5 .5 .5, precision 1 1 2/3 1/2.  Area: two steps of 1/4 under
                # precision 1; eleven points: the six thresholds 0 .. 0.5 see precision 1, the other five nothing
                assert r['tp'][:4] == [2] * 4 and r['fp'][:4] == [2] * 4
                assert r['ap12'][:4] == [0.5] * 4 and r['mAP12'] == 0.5
                assert r['ap07'][:4] == [6.0 / 11.0] * 4 and r['mAP07'] == pytest.approx(6.0 / 11.0, abs=1e-15)


@pytest.mark.timeout_s(600)
def test_end_to_end_through_evaldata_and_a_detect_session(basedir):
    """Darknet-19 VOC-20 with random weights, batch 8, 20 synthetic images of mixed sizes (8 + 8 + 4 padded): every batch's device
    buffers are downloaded and scored by the checker, which isolates the evaluator from the network's numerics."""
    from yolo_tf_amd import evaluate
    from yolo_tf_amd.session import DetectSession
    builder = make_builder(416, basedir)
    sess = DetectSession(builder, 8, dtype='bf16', seed=4)
    m = sess.model
    images, objects, difficult = evaluate.synthetic_dataset(20, 20, seed=9)
    assert len(set(im.shape for im in images)) > 10 and sum(int(d.sum()) for d in difficult) > 0
    data = evaluate.EvalData(images, objects, 8, builder.width, builder.height, m.cell_width, m.cell_height, difficult=difficult)
    for mode, threshold in (('detect', 0.001), ('all', 0.01)):
        want, npos = [], np.zeros(20, np.int64)

        def on_batch(s, gt, base, n_valid):
            r, n = eval_ref.collect(s.conf.cpu().numpy(), s.xy_min.cpu().numpy(), s.xy_max.cpu().numpy(), *data.batch_gt(base, n_valid), base, n_valid,
                                    threshold, 0.5, mode)
            want.extend(r)
            npos[:] += n
        ev = evaluate.Evaluator(20, 20 * sess.N * (20 if mode == 'all' else 1), mode=mode, threshold=threshold, iou_threshold=0.5, keep_curve=True)
        res = evaluate.evaluate(builder, sess, data, mode=mode, threshold=threshold, threshold_iou=0.45, iou=0.5, evaluator=ev, on_batch=on_batch)
        assert len(want) > 100 and res['detections'] == len(want)        # the threshold is low enough for random weights
        assert int(npos.sum()) == sum(int((1 - d).sum()) for d in difficult)
        assert_records_equal(ev.records_numpy(), want)
        assert_result_equal(ev, res, eval_ref.evaluate(want, npos, 20), 20)
