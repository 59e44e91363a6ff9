"""Test-time augmentation through DetectSession and evaluate on the MI355X: tiny-20 with seeded weights at 64x64 (20 boxes) and 96x96 (45),
plain and mirrored.  The fused output is compared bit for bit with the specification (tests/tta_ref.py) applied to what each view left on the
device; a single unflipped view fused at the NMS overlap must score exactly as no augmentation does; and a session without the option owns
none of the new buffers."""
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import tta_ref as T  # noqa: E402

B, CLASSES, STRIDE = 2, 20, 32
OWN = (64, 64)
TTA_ATTRS = ('tta_pooled', 'tta_fused', 'tta_ws', 'tta_rows', 'tta_flags', 'tta_M', 'tta_R')


@pytest.fixture(scope='module')
def basedir():
    with tempfile.TemporaryDirectory() as d:
        yield d


def builder(basedir, size=OWN[0]):
    from bench import make_builder
    return make_builder('tiny', CLASSES, size, False, basedir)[0]


def session(basedir, dtype='f32', **kw):
    from yolo_tf_amd.session import DetectSession
    sess = DetectSession(builder(basedir), B, dtype=dtype, seed=3, **kw)
    e = sess.engine
    e.state.copy_(0.5 + torch.rand(e.state.numel(), device='cuda', generator=torch.Generator(device='cuda').manual_seed(9)))
    e._filters_dirty = True
    return sess


def images_at(w, h):
    return torch.rand(B, h, w, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(100 + w)) * 255


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_fused_views_equal_the_specification(basedir):
    from yolo_tf_amd import tta
    views = tta.parse_views('96 flip', OWN, STRIDE, STRIDE)
    assert views == [(64, 64, False), (96, 96, False), (64, 64, True), (96, 96, True)]
    # seeded weights put most boxes above the threshold in several classes: the rows of an evaluation (a row is one (box, class)), not R = M
    sess = session(basedir, tta=views, tta_rows='evaluation')
    R = 130 * CLASSES
    assert sess.tta == views and sess.tta_M == 2 * (20 + 45) and sess.tta_R == R and sorted(sess.models) == [(64, 64), (96, 96)]
    thr, thr_iou, fuse_iou = 0.02, 0.45, 0.55
    for nms in ('hard', 'gaussian'):
        sess.tta_begin()
        seen = []
        for w, h, flip in views:
            x = images_at(w, h)
            conf, mn, mx = sess.tta_add(x.flip(2).contiguous() if flip else x, (w, h, flip), thr, thr_iou, nms=nms)
            assert conf.shape == (B, (w // STRIDE) * (h // STRIDE) * 5, CLASSES)
            seen.append((conf.cpu().numpy(), mn.cpu().numpy(), mx.cpu().numpy(), w // STRIDE, h // STRIDE, flip))      # before the next view overwrites them
        conf, mn, mx, rows = sess.tta_fuse(thr, fuse_iou, max_per_class=256)
        sess.tta_check()
        assert sess.size == OWN and conf.shape == (B, R, CLASSES) and rows.shape == (B,)
        pooled = T.gather(seen, 2, 2)
        for got, want in zip(sess.tta_pooled, pooled):
            assert np.array_equal(bits(got.cpu().numpy()), bits(want))
        want = T.wbf(*pooled, thr, fuse_iou, len(views), 130, R)
        assert want[4] == 0 and (want[3] > 0).all() and (want[3] < R).all()
        # something was fused: fewer rows than candidates
        assert want[3].sum() < sum(int((s[0] > np.float32(thr)).sum()) for s in seen)
        assert np.array_equal(rows.cpu().numpy(), want[3])
        for got, ref in zip((conf, mn, mx), want[:3]):
            assert np.array_equal(bits(got.cpu().numpy()), bits(ref))


def test_mirrored_evaluation_batch_is_the_mirror_of_the_batch():
    """evaluate's mirrored views rely on it: the resize kernel's flip flag gives the plain batch mirrored, bit for bit, at every size, and
    the ground truth is not touched."""
    from yolo_tf_amd import evaluate
    images, objects, difficult = evaluate.synthetic_dataset(5, CLASSES, seed=4)
    data = evaluate.EvalData(images, objects, B, 64, 64, 2, 2, difficult=difficult, input_sizes=[(64, 64), (96, 96)])
    for w, h in ((64, 64), (96, 96)):
        data.pipe.set_size(w, h)
        for base, n_valid in ((0, 2), (4, 1)):               # (the last batch is padded)
            plain, gt = data.batch(base, n_valid)
            plain = plain.clone()
            mirrored, gt_m = data.batch(base, n_valid, flip=True)
            assert mirrored.shape == (B, h, w, 3) and not torch.equal(mirrored, plain)
            assert torch.equal(mirrored.view(torch.int32), plain.flip(2).contiguous().view(torch.int32))
            assert all(torch.equal(a, b) for a, b in zip(gt, gt_m))
            assert data.batch(base, n_valid, flip=True, with_gt=False)[1] is None


def test_overflow_is_reported_by_tta_check(basedir):
    views = [(64, 64, False), (64, 64, True)]
    sess = session(basedir, tta=views)
    assert sess.tta_R == sess.tta_M == 40                    # the default: as many rows as pooled boxes
    sess.tta_begin()
    for w, h, flip in views:
        sess.tta_add(images_at(w, h), (w, h, flip), 0.0001, 0.45)
    sess.tta_fuse(0.0001, 0.55, max_per_class=1)
    with pytest.raises(RuntimeError, match='max_per_class'):
        sess.tta_check()
    sess.tta_begin()
    sess.tta_check()


class Replay(object):
    """Records what ``session.run`` decodes, call by call, or plays a recording back into the session's buffers: inference sums in arrival order
    and is not repeatable bit for bit, and the invariant below is about everything behind the decode."""

    def __init__(self, sess, recorded=None):
        self.sess, self.real, self.recorded, self.at = sess, sess.run, recorded, 0
        self.out = []

    def __call__(self, images, preprocess_mode=0, check_numerics=True):
        s = self.sess
        if self.recorded is None:
            self.real(images, preprocess_mode, check_numerics=False)
            self.out.append([t.clone() for t in (s.conf, s.xy_min, s.xy_max)])
        else:
            for dst, src in zip((s.conf, s.xy_min, s.xy_max), self.recorded[self.at]):
                dst.copy_(src)
            self.at += 1
        return s.conf, s.xy_min, s.xy_max


@pytest.mark.parametrize('protocol', ['voc', 'coco'])
def test_single_view_at_the_nms_overlap_scores_as_no_augmentation(basedir, protocol):
    """mode 'all': one detection per (box, class), which is what a fused row is; in mode 'detect' a box above the threshold in two classes is
    one detection before the fusion and two rows after it."""
    from yolo_tf_amd import evaluate
    images, objects, difficult = evaluate.synthetic_dataset(5, CLASSES, seed=4)
    thr, thr_iou = 0.005, 0.45
    plain = session(basedir)
    assert not any(hasattr(plain, a) for a in TTA_ATTRS) and plain.tta is None
    data = evaluate.EvalData(images, objects, B, 64, 64, 2, 2, difficult=difficult)
    plain.run = rec = Replay(plain)
    want = evaluate.evaluate(None, plain, data, mode='all', threshold=thr, threshold_iou=thr_iou, protocol=protocol, nms='hard')
    assert len(rec.out) == 3 and want['detections'] > 20 * 5           # more detections than boxes: R = M rows would not hold them
    view = [(64, 64, False)]
    fused = session(basedir, tta=view, tta_rows=20 * CLASSES)
    assert torch.equal(fused.engine.params, plain.engine.params)
    fused.run = Replay(fused, rec.out)
    got = evaluate.evaluate(None, fused, data, mode='all', threshold=thr, threshold_iou=thr_iou, protocol=protocol, nms='hard', tta=view, fuse_iou=thr_iou)
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k]), equal_nan=True), k


def test_session_without_tta_is_what_it_was(basedir):
    plain, views = session(basedir), [(64, 64, False), (64, 64, True)]
    with_tta = session(basedir, tta=views)
    assert plain.tta is None and not any(hasattr(plain, a) for a in TTA_ATTRS) and all(hasattr(with_tta, a) for a in TTA_ATTRS)
    for name in ('tta_begin', 'tta_fuse', 'tta_check'):
        with pytest.raises((AttributeError, TypeError)):
            getattr(plain, name)()
    x = images_at(*OWN)
    decoded = [t.clone() for t in plain.run(x, check_numerics=False)]
    # detect() behind one decoded input: the same NMS launches and the same buffers in both sessions
    outs = []
    for sess in (plain, with_tta):
        sess.run = Replay(sess, [decoded])
        conf, mn, mx, order = sess.detect(x, threshold=0.02, threshold_iou=0.45)
        assert conf.data_ptr() == sess.conf.data_ptr() and conf.shape == (B, 20, CLASSES)
        outs.append([t.clone() for t in (conf, mn, mx, order)])
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*outs))


def test_views_a_session_cannot_serve_are_refused(basedir):
    from yolo_tf_amd.session import DetectSession
    with pytest.raises(ValueError, match='one input size'):
        DetectSession(builder(basedir), B, dtype='int8', calibration=None, tta=[(64, 64, False), (96, 96, False)])
    with pytest.raises(ValueError, match='base view'):
        session(basedir, tta=[(96, 96, False), (64, 64, False)])
    sess = session(basedir, tta=[(64, 64, False), (64, 64, True)])
    with pytest.raises(ValueError):
        sess.tta_add(images_at(96, 96), (96, 96, False))
