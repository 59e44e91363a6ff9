"""Multi-scale training and evaluation on the MI355X: the input pipeline, the training loop, the summaries and the detection session at
several input sizes, each against the single-size code it must not differ from.  tiny-20, batch 2, sizes 64 / 96 / 128 (grids of 2, 3 and
4 cells): the smallest shapes the network takes."""
import configparser
import os
import struct
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

B, CLASSES, STRIDE = 2, 20, 32
SIZES = [(64, 64), (96, 96), (128, 128)]
OWN = (96, 96)


@pytest.fixture(scope='module')
def basedir():
    with tempfile.TemporaryDirectory() as d:
        yield d


@pytest.fixture(scope='module')
def dataset():
    """Eight generated images of different sizes with 1-3 boxes each."""
    rng = np.random.RandomState(8)
    images = [rng.randint(0, 256, (70 + 10 * i, 90 + 7 * i, 3)).astype(np.uint8) for i in range(8)]
    objects = []
    for im in images:
        h, w = im.shape[:2]
        k = rng.randint(1, 4)
        x0, y0 = rng.uniform(0, 0.5 * w, k), rng.uniform(0, 0.5 * h, k)
        objects.append((rng.randint(0, CLASSES, k), np.stack([x0, y0, x0 + rng.uniform(8, 0.4 * w, k), y0 + rng.uniform(8, 0.4 * h, k)], 1)))
    return images, objects


def augment_config():
    """config.ini's two augmentation sections with every augmentation enabled, and applied to every image where a probability decides."""
    ini = configparser.ConfigParser()
    ini.read(os.path.join(ROOT, 'config.ini'))
    from yolo_tf_amd.utils.augment import AugmentConfig
    cfg = AugmentConfig(ini)
    assert cfg.full_enable and cfg.random_crop > 0 and cfg.resized_enable
    assert cfg.flip and cfg.brightness and cfg.contrast and cfg.saturation and cfg.hue and cfg.noise and cfg.grayscale_probability > 0
    cfg.full_probability = cfg.probability = 1.0
    return cfg


def builder(training, basedir, size=OWN[0]):
    from bench import make_builder
    return make_builder('tiny', CLASSES, size, training, basedir)[0]


def multi_pipeline(dataset, seed):
    from yolo_tf_amd.utils.augment import DeviceInputPipeline
    return DeviceInputPipeline(dataset[0], dataset[1], B, OWN[0], OWN[1], CLASSES, OWN[0] // STRIDE, OWN[1] // STRIDE, config=augment_config(), seed=seed,
                               sizes=SIZES, downsampling=(STRIDE, STRIDE))


def fixed_pipelines(dataset, seed=0):
    """One pipeline per size, built the way the single-size code builds it."""
    from yolo_tf_amd.utils.augment import DeviceInputPipeline
    return {(w, h): DeviceInputPipeline(dataset[0], dataset[1], B, w, h, CLASSES, w // STRIDE, h // STRIDE, config=augment_config(), seed=seed)
            for w, h in SIZES}


class LabelHolder(object):
    """What DeviceInputPipeline.next reads of a session: the current size and the six label buffers of its grid."""

    def __init__(self):
        from yolo_tf_amd.session import _label_shapes
        self._labels = {(w, h): [torch.full(s, 7.0, dtype=torch.float32, device='cuda') for s in _label_shapes(B, (w // STRIDE) * (h // STRIDE), CLASSES)]
                        for w, h in SIZES}
        self.set_size(*OWN)

    def set_size(self, w, h):
        self.size, self.labels = (w, h), self._labels[(w, h)]


def bits(t):
    return t.contiguous().view(torch.int32)


def test_pipeline_at_each_size_is_bitwise_the_fixed_size_pipeline(dataset):
    multi, fixed = multi_pipeline(dataset, seed=2), fixed_pipelines(dataset)
    assert multi.buffer.shape == (B * 128 * 128 * 3,)                    # allocated once, for the largest size
    held, ref = LabelHolder(), LabelHolder()
    flags = set()
    for w, h in [(64, 64), (128, 128), (64, 64)]:
        one = fixed[(w, h)]
        one.rng.set_state(multi.rng.get_state())
        held.set_size(w, h)
        ref.set_size(w, h)
        multi.buffer.fill_(float('nan'))
        got = multi.next(held)
        want = one.next(ref)
        torch.cuda.synchronize()
        multi.check()
        assert got.shape == (B, h, w, 3) and got.is_contiguous() and got.data_ptr() == multi.buffer.data_ptr()
        assert (multi.cell_width, multi.cell_height) == (w // STRIDE, h // STRIDE)
        assert not torch.isnan(got).any()
        assert torch.equal(bits(got), bits(want))
        assert torch.isnan(multi.buffer[got.numel():]).all()              # nothing is written past the view
        for i, (x, y) in enumerate(zip(held.labels, ref.labels)):
            assert x.shape == y.shape and torch.equal(bits(x), bits(y)), 'label tensor %d at %dx%d' % (i, w, h)
        assert float(held.labels[0].sum()) >= 1
        # the host draws consumed the generator exactly as the fixed-size pipeline's did
        a, b = multi.rng.get_state(), one.rng.get_state()
        assert np.array_equal(a[1], b[1]) and a[2:] == b[2:]
        flags |= set(int(p.flags) for p in multi.assemble(multi.sample())[0])
    assert any(f & 32 for f in flags) and any(f & 16 for f in flags)      # noise and contrast were among what was compared


def test_pipeline_without_sizes_allocates_one_batch_of_its_shape(dataset):
    one = fixed_pipelines(dataset)[(96, 96)]
    assert one.out.shape == (B, 96, 96, 3) and one.buffer is one.out and one.out.untyped_storage().nbytes() == B * 96 * 96 * 3 * 4
    held = LabelHolder()
    held.set_size(64, 64)                                                 # a single-size pipeline never looks at the session's size
    assert one.next(held).shape == (B, 96, 96, 3)
    with pytest.raises(KeyError):
        one.set_size(64, 64)
    with pytest.raises(KeyError):
        multi_pipeline(dataset, 0).set_size(160, 160)


def session_state(sess):
    e = sess.engine
    return [e.params.clone(), e.state.clone()] + [s.clone() for s in sess.optimizer.slots]


def train_session(b, sizes=SIZES):
    from yolo_tf_amd.session import TrainSession
    return TrainSession(b, B, dtype='f32', optimizer='adam', learning_rate=1e-3, seed=4, deterministic=True, sizes=sizes)


def test_training_loop_follows_the_schedule_bitwise_reproducibly(dataset, basedir):
    from yolo_tf_amd import multiscale
    b = builder(True, basedir)
    schedule = multiscale.SizeSchedule(SIZES, 2, 0)
    want = [schedule.at(g) for g in range(8)]
    assert len(set(want)) == 3                                            # (seed 0 visits all three sizes in eight steps)

    def run():
        sess, pipe, visited = train_session(b), multi_pipeline(dataset, seed=3), []
        assert sess.size == OWN and sorted(sess.models) == SIZES
        for _ in range(8):
            assert multiscale.follow(sess, schedule) == sess.size
            visited.append(sess.size)
            sess.step(pipe.next(sess))
        torch.cuda.synchronize()
        pipe.check()
        assert sess.global_step == 8 and np.isfinite(sess.fetch()['total_loss'])
        return visited, session_state(sess)
    (v0, s0), (v1, s1) = run(), run()
    assert v0 == want and v1 == want
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(s0, s1))
    assert torch.isfinite(s0[0]).all()
    # by hand: set_size and the fixed-size pipelines, all drawing from one generator
    sess, fixed = train_session(b), fixed_pipelines(dataset)
    rng = np.random.RandomState(3)
    for p in fixed.values():
        p.rng = rng
    for g in range(8):
        sess.set_size(*want[g])
        sess.step(fixed[want[g]].next(sess))
    torch.cuda.synchronize()
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(s0, session_state(sess)))


def test_key_absent_one_size_and_the_buffer_of_today(dataset, basedir):
    import train
    from yolo_tf_amd import multiscale, utils
    cfg = utils.make_config([os.path.join(ROOT, 'config.ini'), os.path.join(ROOT, 'config', 'yolo2', 'tiny-20.ini')])
    assert train.multiscale_setting(train.make_args(['--data', 'synthetic']), cfg) is None
    sess = train_session(builder(True, basedir), sizes=None)
    assert list(sess.models) == [OWN] and len(sess.engine._bindings) == 1
    data = train.DeviceAugmentedData(dataset, B, 96, 96, CLASSES, 3, 3, augment_config(), 0, 0, 1, sess, sizes=None, downsampling=None)
    assert data.pipe.out.shape == (B, 96, 96, 3) and data.pipe.out.untyped_storage().nbytes() == B * 96 * 96 * 3 * 4 and data.pipe._views is None
    assert multiscale.follow(sess, None) == OWN
    images, labels = data.next()
    assert images.shape == (B, 96, 96, 3) and labels is None
    synthetic = train.SyntheticData(B, CLASSES, 96, 96, 3, 3, 1)
    images, labels = synthetic.next()
    assert images.shape == (B, 96, 96, 3) and labels[0].shape[1] == 9
    # with a session, synthetic data follows its size
    multi = train_session(builder(True, basedir))
    synthetic = train.SyntheticData(B, CLASSES, 96, 96, 3, 3, 1, session=multi, downsampling=(STRIDE, STRIDE))
    for w, h in [(64, 64), (128, 128)]:
        multi.set_size(w, h)
        images, labels = synthetic.next()
        assert images.shape == (B, h, w, 3) and labels[0].shape[1] == (w // STRIDE) * (h // STRIDE)
        multi.step(images, labels)
    assert np.isfinite(multi.fetch()['total_loss'])


def png_size(data):
    assert data[:8] == b'\x89PNG\r\n\x1a\n' and data[12:16] == b'IHDR'
    return struct.unpack('>II', data[16:24])


def test_summaries_follow_the_size_of_the_step(dataset, basedir):
    from yolo_tf_amd.session import TrainSession
    from yolo_tf_amd.summary import HistogramSummaries, ImageSummaries
    cfg = configparser.ConfigParser()
    cfg.add_section('summary')
    cfg.set('summary', 'image', r'[_\w\d]+\/input$')
    cfg.set('summary', 'image_max', '1')
    cfg.set('summary', 'histogram', r'[_\w\d]+\/input$')
    sess = TrainSession(builder(True, basedir), B, dtype='bf16', optimizer='adam', learning_rate=1e-3, seed=4, sizes=SIZES)
    pipe = multi_pipeline(dataset, seed=5)
    images_summary, histograms = ImageSummaries(sess, cfg), HistogramSummaries(sess, cfg)

    class Writer(object):
        def add_images(self, step, images):
            self.images = images

    for w, h in [(64, 64), (128, 128), (64, 64)]:
        sess.set_size(w, h)
        sess.step(pipe.next(sess))
        images_summary.collect()
        histograms.collect()
        writer = Writer()
        assert images_summary.write(writer, sess.global_step) == 1
        (tag, proto), = writer.images
        assert tag == 'yolo2_tiny/input/image' and (proto['width'], proto['height'], proto['colorspace']) == (w, h, 3)
        assert png_size(proto['encoded_image_string']) == (w, h)
        (htag, record), = histograms.results()[0]
        assert htag == 'yolo2_tiny/input' and record['num'] == B * h * w * 3


def detect_session(b, dtype, sizes=None):
    from yolo_tf_amd.session import DetectSession
    return DetectSession(b, B, dtype=dtype, seed=3, sizes=sizes)


def moving_statistics(n):
    """Moving means and variances that are not the initial 0 and 1 (all positive: one draw serves both)."""
    return 0.5 + torch.rand(n, device='cuda', generator=torch.Generator(device='cuda').manual_seed(9))


def detect_images(s):
    return torch.rand(B, s, s, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(100 + s)) * 255


def single_session(basedir, dtype, s):
    sess = detect_session(builder(False, basedir, s), dtype)
    sess.engine.state.copy_(moving_statistics(sess.engine.state.numel()))
    sess.engine._filters_dirty = True
    return sess


def run_outputs(sess, images):
    """conf, xy_min, xy_max of one forward and decode, before the NMS."""
    sess.run(images, check_numerics=False)
    torch.cuda.synchronize()
    return [t.clone() for t in (sess.conf, sess.xy_min, sess.xy_max)]


def nms_outputs(sess, decoded):
    """The NMS of ``decoded`` (conf, xy_min, xy_max), run in ``sess``'s own buffers: (conf after it, order)."""
    for dst, src in zip((sess.conf, sess.xy_min, sess.xy_max), decoded):
        dst.copy_(src)
    order = sess.nms(threshold=0.0001, threshold_iou=0.4)
    torch.cuda.synchronize()
    return bits(sess.conf).clone(), order.clone()


# Inference is NOT bitwise repeatable on the code before this feature: two single-size sessions of one process, and two runs of one session, differ
# (the convolutions add K-sliced partial sums with f32 atomics in arrival order; in bf16 a sum that lands on the other side of a rounding boundary
# then moves an activation by one bf16 ulp, and the layers behind it carry that on).  Measured on these very inputs (SPREAD_RUNS forward + decode
# runs per dtype and size over three single-size sessions, every run against the first three; profiles/multiscale.md): the largest absolute
# difference of conf and of xy_min / xy_max over the three sizes, before the NMS.  The comparisons of decoded outputs below allow TWICE this
# spread.  The NMS itself is repeatable, so it is compared bit for bit on one and the same decoded input: after it, a score next to the threshold or
# two boxes next to the overlap limit turn the spread above into kept / suppressed (13 of 59 bf16 runs at 128 ordered differently).
SPREAD_RUNS = 60
SPREAD = {'f32': (2.7e-7, 4.4e-5), 'bf16': (4.6e-4, 0.055)}       # dtype: (conf, xy_min / xy_max); conf reaches 0.17, the coordinates 23 cells


def assert_within_spread(got, want, dtype, what):
    conf_tol, xy_tol = (2 * v for v in SPREAD[dtype])
    for name, x, y, tol in zip(('conf', 'xy_min', 'xy_max'), got, want, (conf_tol, xy_tol, xy_tol)):
        assert x.shape == y.shape and torch.isfinite(x).all() and torch.isfinite(y).all(), (name, what)
        err = float((x - y).abs().max())
        print('%s %s %s: max abs difference %.3e (allowed %.3e)' % (what, dtype, name, err, tol))
        assert err <= tol, '%s of %s: %.3e > %.3e' % (name, what, err, tol)


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
def test_two_single_size_sessions_agree_within_the_recorded_spread(basedir, dtype):
    """The premise of the next test.  Expected: bitwise equality.  Found: not so on the code before this feature (see SPREAD); what holds is twice the
    spread for the decoded outputs, and bitwise equality for the NMS of one decoded input."""
    for s in (64, 96, 128):
        images = detect_images(s)
        first, second = single_session(basedir, dtype, s), single_session(basedir, dtype, s)          # (both alive: different addresses)
        decoded = run_outputs(first, images)
        assert_within_spread(decoded, run_outputs(second, images), dtype, 'two single-size sessions at %d' % s)
        (c0, o0), (c1, o1) = nms_outputs(first, decoded), nms_outputs(second, decoded)
        assert torch.equal(c0, c1) and torch.equal(o0, o1)


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
def test_detect_session_at_several_sizes_equals_single_size_sessions(basedir, dtype):
    multi = detect_session(builder(False, basedir), dtype, sizes=SIZES)
    e = multi.engine
    e.state.copy_(moving_statistics(e.state.numel()))
    e._filters_dirty = True
    assert multi.size == OWN and sorted(multi.models) == SIZES
    storage = multi.conf.untyped_storage().data_ptr()
    for s in (128, 64, 96):
        images = detect_images(s)
        multi.set_size(s, s)
        n = (s // STRIDE) ** 2 * multi.A
        assert multi.N == n and multi.conf.shape == (B, n, CLASSES) and multi.conf.is_contiguous() and multi.order.shape == (B, n)
        assert multi.conf.untyped_storage().data_ptr() == storage          # views of the one allocation
        assert multi.model.cell_width == s // STRIDE and multi.model.conf.shape == (B, (s // STRIDE) ** 2, multi.A, CLASSES)
        got = run_outputs(multi, images)
        assert multi.model.iou.shape == (B, (s // STRIDE) ** 2, multi.A)
        single = single_session(basedir, dtype, s)
        assert torch.equal(single.engine.params, e.params) and torch.equal(single.engine.state, e.state)       # the same variables (same seed)
        want = run_outputs(single, images)
        assert_within_spread(got, want, dtype, 'several sizes against one, at %d' % s)
        # the NMS of the single-size session's decoded outputs, in the views of the shared buffers and in the single-size buffers
        (conf_multi, order_multi), (conf_single, order_single) = nms_outputs(multi, want), nms_outputs(single, want)
        assert torch.equal(conf_multi, conf_single) and torch.equal(order_multi, order_single), 'NMS at %d' % s
        kept = (conf_multi.view(torch.float32) > 0).sum()
        assert 0 < kept < (want[0] > 0).sum()                              # it kept something and suppressed something
        # and detect() as a whole: the same launches in one call
        conf, _, _, order = multi.detect(images, threshold=0.0001, threshold_iou=0.4)
        assert conf.data_ptr() == multi.conf.data_ptr() and order.shape == (B, n)
    with pytest.raises(KeyError):
        multi.set_size(160, 160)


def test_int8_with_sizes_is_refused(basedir):
    from yolo_tf_amd.session import DetectSession
    with pytest.raises(ValueError) as e:
        DetectSession(builder(False, basedir), B, dtype='int8', calibration=None, sizes=SIZES)
    assert 'one input size' in str(e.value)


def test_eval_data_walks_one_upload_at_each_size(dataset, basedir):
    from yolo_tf_amd import evaluate
    images, objects = dataset
    difficult = [np.arange(len(c)) % 2 == 1 for c, _ in objects]
    multi = evaluate.EvalData(images, objects, B, 96, 96, 3, 3, difficult=difficult, input_sizes=SIZES)
    sess = detect_session(builder(False, basedir), 'bf16', sizes=SIZES)
    src = multi.pipe.src.data_ptr()
    for s in (128, 64):
        one = evaluate.EvalData(images, objects, B, s, s, s // STRIDE, s // STRIDE, difficult=difficult)
        multi.set_size(s, s)
        sess.set_size(s, s)
        assert multi.pipe.src.data_ptr() == src and len(multi) == len(one) == 4
        for protocol in ('voc', 'coco'):
            for (xa, ga, ba, na), (xb, gb, bb, nb) in zip(multi.batches(protocol), one.batches(protocol)):
                assert xa.shape == (B, s, s, 3) and xa.is_contiguous() and torch.equal(bits(xa), bits(xb)) and (ba, na) == (bb, nb)
                assert len(ga) == len(gb) and all(torch.equal(p, q) for p, q in zip(ga, gb))
        result = evaluate.evaluate(None, sess, multi, mode='all', threshold=0.0001)       # the two walk together (scores: tests/test_multiscale_cli_gpu.py)
        assert len(result['ap07']) == CLASSES and sum(result['npos']) == sum(int((~d).sum()) for d in difficult) and result['detections'] > 0      # (difficult boxes do not count)
