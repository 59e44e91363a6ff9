"""Image summaries without a GPU: known answers of the specification (tests/image_summary_ref.py) on hand-computed 2x2 images, tag naming,
the PNG container (this project's decoder and, independently, PIL), the event encoding (this project's decoder and google.protobuf),
unchanged bytes of events without images, and name resolution of the reference's pattern against graphs built on the host."""
import configparser
import logging
import os
import sys
import tempfile
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_summary_ref as R  # noqa: E402
import summary_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the reference's commented image pattern (config.ini:66 there)
PATTERN = r'[_\w\d]+\/(input|conv\d*\/(convolution|leaky_relu\/data))$'
NAN, INF = np.nan, np.inf


def _img(values, depth=1):
    return np.array(values, np.float32).reshape(2, 2, depth)


def test_non_negative_image_maps_its_max_to_255():
    out, info = R.normalize_image(_img([0.0, 1.0, 2.0, 4.0]))
    assert out.reshape(-1).tolist() == [0, 63, 127, 255]            # 255 / 4 = 63.75: 63.75 -> 63, 127.5 -> 127
    assert (info['min'], info['max'], info['scale'], info['offset'], info['nonfinite']) == (0.0, 4.0, 63.75, 0.0, 0)


def test_mixed_sign_image_maps_zero_to_128():
    out, info = R.normalize_image(_img([-2.0, 0.0, 1.0, 2.0]))
    assert out.reshape(-1).tolist() == [1, 128, 191, 255]           # 127 / 2 = 63.5: -127 + 128, 128, 63.5 + 128 -> 191, 127 + 128
    assert (info['min'], info['max'], info['scale'], info['offset']) == (-2.0, 2.0, 63.5, 128.0)
    out, info = R.normalize_image(_img([-4.0, 0.0, 1.0, 2.0]))      # m is |image_min| here
    assert out.reshape(-1).tolist() == [1, 128, 159, 191] and info['scale'] == 31.75


def test_all_zero_and_tiny_images_have_scale_zero():
    out, info = R.normalize_image(_img([0.0] * 4))
    assert out.reshape(-1).tolist() == [0] * 4 and info['scale'] == 0.0 and info['offset'] == 0.0
    out, info = R.normalize_image(_img([0.0, 1e-7, 5e-7, 9.9e-7]))
    assert out.reshape(-1).tolist() == [0] * 4 and info['scale'] == 0.0
    out, info = R.normalize_image(_img([-9e-7, 1e-7, 0.0, 5e-7]))   # negative minimum: offset 128 with scale 0
    assert out.reshape(-1).tolist() == [128] * 4 and info['scale'] == 0.0 and info['offset'] == 128.0
    out, info = R.normalize_image(_img([0.0, 2e-6, 1e-6, 0.0]))     # just above the threshold: scaled
    assert out.reshape(-1).tolist() == [0, 255, 127, 0]


def test_non_finite_pixels_become_the_bad_colour_and_leave_min_max_alone():
    out, info = R.normalize_image(_img([NAN, 1.0, 2.0, INF]))
    assert out.reshape(-1).tolist() == [255, 127, 255, 255] and (info['min'], info['max'], info['nonfinite']) == (1.0, 2.0, 2)
    # three channels: one bad value spoils its whole pixel, and that pixel's other values do not reach min / max
    x = _img([1.0, 2.0, 4.0, -INF, 100.0, -100.0, 0.0, 0.0, 0.0, 2.0, NAN, 2.0], depth=3)
    out, info = R.normalize_image(x)
    assert out.reshape(4, 3).tolist() == [[63, 127, 255], [255, 0, 0], [0, 0, 0], [255, 0, 0]]
    assert (info['min'], info['max'], info['nonfinite']) == (0.0, 4.0, 2)
    out, info = R.normalize_image(_img([1.0] * 12 + [NAN, 1.0, 1.0, 1.0], depth=4))
    assert out.reshape(4, 4)[3].tolist() == [255, 0, 0, 255] and out.reshape(4, 4)[0].tolist() == [255] * 4


def test_every_pixel_non_finite():
    out, info = R.normalize_image(_img([NAN, INF, -INF, NAN]))
    assert out.reshape(-1).tolist() == [255] * 4
    assert (info['min'], info['max'], info['scale'], info['offset'], info['nonfinite']) == (INF, -INF, 0.0, 0.0, 4)
    out, _ = R.normalize_image(_img([NAN] * 12, depth=3))
    assert out.reshape(4, 3).tolist() == [[255, 0, 0]] * 4


@pytest.mark.parametrize('c', [2, 5])
def test_other_channel_counts_are_summed_to_depth_one(c):
    x = np.arange(2 * 2 * 2 * c, dtype=np.float32).reshape(2, 2, 2, c)
    (tag, out, info), = R.image_summary('t', x, 1)
    assert tag == 't/image' and out.shape == (2, 2, 1)
    sums = x[0].sum(-1)                                             # small integers: exact in any order
    assert np.array_equal(R.channel_sum(x[0]), sums)
    assert np.array_equal(out[..., 0], np.trunc(sums * (np.float32(255) / sums.max())).astype(np.uint8))
    assert info['max'] == float(sums.max()) and out.max() == 255


def test_channel_sum_order_and_single_rounding():
    # 1 + 2^-30 nine times: f32 accumulation would lose every small term, f64 keeps them and rounds once
    x = np.array([1.0] + [2.0 ** -30] * 8 + [2.0 ** -24], np.float32)
    assert R.channel_sum(x) == np.float32(1.0 + 8 * 2.0 ** -30 + 2.0 ** -24) and R.channel_sum(x) != np.float32(1.0)
    # the order shows: 2^60 in group 0, -2^60 in group 1, small values around them
    y = np.zeros(16, np.float32)
    y[0], y[1], y[8], y[9] = 2.0 ** 60, 1.0, -2.0 ** 60, 1.0
    assert R.channel_sum(y) == 0.0                                   # (2^60 + 1) -> 2^60 and (-2^60 + 1) -> -2^60 inside the groups
    z = np.zeros(16, np.float32)
    z[0], z[7], z[8] = 2.0 ** 60, -2.0 ** 60, 1.0
    assert R.channel_sum(z) == 1.0                                   # cancels inside group 0, the 1 survives
    assert R.channel_sum(np.array([-0.0, -0.0], np.float32)).tobytes() == np.float32(0.0).tobytes()      # the chains start at +0.0


@pytest.mark.parametrize('c', [1, 3, 4])
def test_image_channel_counts_are_kept(c):
    rng = np.random.RandomState(c)
    x = rng.standard_normal((3, 2, 2, c)).astype(np.float32)
    res = R.image_summary('t', x, 2)
    assert [r[0] for r in res] == ['t/image/0', 't/image/1'] and all(r[1].shape == (2, 2, c) for r in res)
    out0, _ = R.normalize_image(x[0])
    assert np.array_equal(res[0][1], out0)


def test_bf16_input_is_widened():
    bits = np.array([0x3f80, 0x4000, 0x0000, 0x7fc0], np.uint16).reshape(1, 2, 2, 1)      # 1, 2, 0, NaN
    (_, out, info), = R.image_summary('t', bits, 1)
    assert out.reshape(-1).tolist() == [127, 255, 0, 255] and info['nonfinite'] == 1


def test_tags_and_image_max():
    from yolo_tf_amd import summary
    for fn in (R.tags, summary.image_tags):
        assert fn('a/input', 1, 4) == ['a/input/image'] and fn('a/input', 1, 1) == ['a/input/image']
        assert fn('a/input', 3, 2) == ['a/input/image/0', 'a/input/image/1']
        assert fn('a/input', 3, 5) == ['a/input/image/0', 'a/input/image/1', 'a/input/image/2']
    with pytest.raises(ValueError):
        R.tags('a', 0, 2)
    with pytest.raises(ValueError):
        summary.ImageSummaries(None, _config(PATTERN, 0))
    with pytest.raises(ValueError):
        R.image_summary('a', np.zeros((1, 2, 2, 1), np.float32), 0)


@pytest.mark.parametrize('depth', [1, 3, 4])
def test_png_round_trip(depth):
    from yolo_tf_amd.utils import png
    rng = np.random.RandomState(depth)
    img = rng.randint(0, 256, (5, 7, depth)).astype(np.uint8)
    data = png.encode(img)
    assert np.array_equal(png.decode(data), img)
    # the container as the specification states it: IHDR fields, filter type 0 on every row -- readable with zlib alone
    assert data[:8] == b'\x89PNG\r\n\x1a\n' and data[12:16] == b'IHDR'
    assert tuple(data[16:29]) == (0, 0, 0, 7, 0, 0, 0, 5, 8, {1: 0, 3: 2, 4: 6}[depth], 0, 0, 0)
    i = data.index(b'IDAT')
    n = int.from_bytes(data[i - 4:i], 'big')
    raw = np.frombuffer(zlib.decompress(data[i + 4:i + 4 + n]), np.uint8).reshape(5, 1 + 7 * depth)
    assert not raw[:, 0].any() and np.array_equal(raw[:, 1:].reshape(5, 7, depth), img)
    with pytest.raises(ValueError):
        png.decode(data[:40] + bytes([data[40] ^ 1]) + data[41:])     # a flipped bit: the CRC says so
    if depth == 1:
        assert np.array_equal(png.decode(png.encode(img[:, :, 0])), img)


@pytest.mark.parametrize('depth', [1, 3, 4])
def test_png_reads_with_pil(depth):
    Image = pytest.importorskip('PIL.Image')
    import io
    from yolo_tf_amd.utils import png
    rng = np.random.RandomState(10 + depth)
    img = rng.randint(0, 256, (6, 9, depth)).astype(np.uint8)
    im = Image.open(io.BytesIO(png.encode(img)))
    assert im.mode == {1: 'L', 3: 'RGB', 4: 'RGBA'}[depth] and im.size == (9, 6)
    assert np.array_equal(np.asarray(im).reshape(6, 9, depth), img)


def _images():
    from yolo_tf_amd.utils import png
    rng = np.random.RandomState(0)
    out = []
    for tag, (h, w, d) in (('s/input/image', (4, 6, 3)), ('s/conv0/convolution/image', (3, 5, 1)), ('s/rgba/image/1', (2, 2, 4))):
        pix = rng.randint(0, 256, (h, w, d)).astype(np.uint8)
        out.append((tag, {'height': h, 'width': w, 'colorspace': d, 'encoded_image_string': png.encode(pix)}, pix))
    return out


def test_event_round_trip_with_images():
    from yolo_tf_amd.utils import events, png
    ims = _images()
    images = [(t, d) for t, d, _ in ims]
    scalars = [('total_loss', 1.5)]
    h = {'min': -1.0, 'max': 2.0, 'num': 3.0, 'sum': 1.0, 'sum_squares': 5.0, 'bucket_limit': [1.0, S.DBL_MAX], 'bucket': [3.0, 0.0]}
    buf = events.encode_event(3.25, step=9, scalars=scalars, histograms=[('w', h)], images=images)
    ev = events.decode_event(buf)
    assert ev['step'] == 9 and ev['scalars'] == scalars and ev['histograms'] == [('w', h)]       # image values do not land in the scalars
    assert ev['images'] == images
    for (_, d), (_, _, pix) in zip(ev['images'], ims):
        assert np.array_equal(png.decode(d['encoded_image_string']), pix)
    only = events.decode_event(events.encode_event(1.0, step=2, images=images))
    assert only['scalars'] == [] and only['histograms'] == [] and only['images'] == images
    # through a file
    w = events.FileWriter(tempfile.mkdtemp(prefix='image_events_'))
    w.add_scalars(1, scalars)
    w.add_images(2, images)
    w.close()
    evs = events.read_events(w.path)
    assert evs[1]['scalars'] == scalars and evs[1]['images'] == []
    assert evs[2]['step'] == 2 and evs[2]['images'] == images and evs[2]['scalars'] == []


def test_events_without_images_keep_their_bytes():
    from yolo_tf_amd.utils import events
    scalars = [('total_loss', 1.5), ('a/gradient_norm', 0.25)]
    h = {'min': 0.0, 'max': 0.0, 'num': 7.0, 'sum': 0.0, 'sum_squares': 0.0, 'bucket_limit': [1e-12, S.DBL_MAX], 'bucket': [7.0, 0.0]}
    # recorded from the encoder before it knew images: wall_time 1.0, step 3; the two scalars, then one scalar and the histogram
    assert events.encode_event(1.0, step=3, scalars=scalars).hex() == (
        '09000000000000f03f10032a2b0a110a0a746f74616c5f6c6f7373150000c03f0a160a0f612f6772616469656e745f6e6f726d150000803e')
    assert events.encode_event(1.0, step=3, scalars=[('n', 2.0)], histograms=[('z', h)]).hex() == (
        '09000000000000f03f10032a3e0a080a016e15000000400a320a017a2a2d190000000000001c40321011ea2d819997713dffffffffffffef7f3a10'
        '0000000000001c400000000000000000')
    for kw in ({'scalars': scalars}, {'scalars': scalars, 'histograms': [('z', h)]}, {'histograms': [('z', h)]}, {'file_version': 'brain.Event:2'}, {}):
        assert events.encode_event(1.0, step=3, **kw) == events.encode_event(1.0, step=3, images=None, **kw)
        assert events.encode_event(1.0, step=3, **kw) == events.encode_event(1.0, step=3, images=[], **kw)
        assert events.decode_event(events.encode_event(1.0, step=3, **kw))['images'] == []


def _event_message_class():
    """tensorflow.Event / Summary / Summary.Image rebuilt from descriptors: an independent reader of the bytes."""
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name='image_summary_test.proto', package='tfimgtest', syntax='proto3')
    im = fd.message_type.add(name='Image')
    for i, n in enumerate(('height', 'width', 'colorspace'), 1):
        im.field.add(name=n, number=i, type=F.TYPE_INT32, label=F.LABEL_OPTIONAL)
    im.field.add(name='encoded_image_string', number=4, type=F.TYPE_BYTES, label=F.LABEL_OPTIONAL)
    v = fd.message_type.add(name='Value')
    v.field.add(name='tag', number=1, type=F.TYPE_STRING, label=F.LABEL_OPTIONAL)
    v.field.add(name='simple_value', number=2, type=F.TYPE_FLOAT, label=F.LABEL_OPTIONAL)
    v.field.add(name='image', number=4, type=F.TYPE_MESSAGE, label=F.LABEL_OPTIONAL, type_name='.tfimgtest.Image')
    s = fd.message_type.add(name='Summary')
    s.field.add(name='value', number=1, type=F.TYPE_MESSAGE, label=F.LABEL_REPEATED, type_name='.tfimgtest.Value')
    e = fd.message_type.add(name='Event')
    e.field.add(name='wall_time', number=1, type=F.TYPE_DOUBLE, label=F.LABEL_OPTIONAL)
    e.field.add(name='step', number=2, type=F.TYPE_INT64, label=F.LABEL_OPTIONAL)
    e.field.add(name='summary', number=5, type=F.TYPE_MESSAGE, label=F.LABEL_OPTIONAL, type_name='.tfimgtest.Summary')
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    desc = pool.FindMessageTypeByName('tfimgtest.Event')
    if hasattr(message_factory, 'GetMessageClass'):
        return message_factory.GetMessageClass(desc)
    return message_factory.MessageFactory(pool).GetPrototype(desc)


def test_event_bytes_parse_with_protobuf():
    pytest.importorskip('google.protobuf')
    from yolo_tf_amd.utils import events
    ims = _images()
    buf = events.encode_event(12.5, step=7, scalars=[('total_loss', 1.5)], images=[(t, d) for t, d, _ in ims])
    msg = _event_message_class()()
    msg.ParseFromString(buf)
    assert msg.step == 7 and len(msg.summary.value) == 4 and msg.summary.value[0].simple_value == 1.5
    for v, (tag, d, _) in zip(msg.summary.value[1:], ims):
        assert v.tag == tag and v.HasField('image')
        assert (v.image.height, v.image.width, v.image.colorspace, v.image.encoded_image_string) == (d['height'], d['width'], d['colorspace'], d['encoded_image_string'])
    assert msg.SerializeToString() == buf            # and protobuf writes the same bytes back


def _graph(inference):
    sys.path.insert(0, ROOT)
    from bench import make_builder
    b, _ = make_builder(inference, 20, 96, True, tempfile.mkdtemp(prefix='image_summary_graph_'))
    return b.graph


class _FakeSession(object):
    def __init__(self, graph):
        self.engine = type('E', (), {'graph': graph})()


def _config(image=None, image_max=None, section=True, key='image'):
    c = configparser.ConfigParser()
    if section:
        c.add_section('summary')
        if image is not None:
            c.set('summary', key, image)
        if image_max is not None:
            c.set('summary', 'image_max', str(image_max))
    return c


@pytest.mark.parametrize('inference,scope,convs', [('darknet', 'yolo2_darknet', 22), ('tiny', 'yolo2_tiny', 9)])
def test_reference_pattern_selects_input_and_conv_tensors(inference, scope, convs):
    from yolo_tf_amd.summary import ImageSummaries
    g = _graph(inference)
    bn = convs - 1
    s = ImageSummaries(_FakeSession(g), _config(PATTERN, 1))
    assert s.enabled and s.image_max == 1
    names = [n for n, _ in s.resolve()]
    # (the last layer, scope plain `conv`, has biases and no activation: its output is `conv/BiasAdd`, which the pattern does not name)
    want = ['%s/input' % scope] + ['%s/conv%d/%s' % (scope, i, k) for i in range(bn) for k in ('convolution', 'leaky_relu/data')]
    assert sorted(names) == sorted(want) and names[0] == '%s/input' % scope
    tensors = dict(s.resolve())
    assert tensors['%s/input' % scope].c == 3 and tensors['%s/conv0/convolution' % scope].c in (16, 32)


def test_key_handling_and_disabled_default(caplog):
    from yolo_tf_amd.summary import ImageSummaries
    g = _graph('tiny')
    own = configparser.ConfigParser()
    own.read(os.path.join(ROOT, 'config.ini'))
    spelled = _config(PATTERN, 1, key='image_')                      # the reference's default config spells the key `image_`
    for cfg in (_config(), _config(section=False), None, spelled, _config(PATTERN), _config(image_max=3), own):
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            s = ImageSummaries(_FakeSession(g), cfg)
        assert not s.enabled and s.pattern is None
        assert [r.getMessage() for r in caplog.records] == ['summary_image disabled']       # one warning, as the reference's
        s.collect()                                  # disabled: returns before it touches torch or the device
        assert s._plans == {} and s.results() == [] and s.resolve() == []
    s = ImageSummaries(_FakeSession(g), _config(PATTERN, 4))
    assert s.enabled and s.image_max == 4


def test_matched_variables_are_skipped_with_one_warning(caplog):
    from yolo_tf_amd.summary import ImageSummaries
    g = _graph('tiny')
    s = ImageSummaries(_FakeSession(g), _config(r'.*/conv0/.*', 1))
    with caplog.at_level(logging.WARNING):
        names = [n for n, _ in s.resolve()]
        again = [n for n, _ in s.resolve()]
    assert names == again and 'yolo2_tiny/conv0/convolution' in names
    assert not [n for n in names if n.endswith('/weights') or 'BatchNorm' in n]
    msgs = [r.getMessage() for r in caplog.records if 'not images' in r.getMessage()]
    assert len(msgs) == 1 and 'yolo2_tiny/conv0/weights' in msgs[0]


def test_host_queries_and_argument_errors_without_a_gpu():
    """Host-only parts of the C ABI: depth, the static work split of a job, the sizes, and the argument checks."""
    from yolo_tf_amd import _lib
    q = _lib.query
    assert [q('yolo2_image_summary_depth', c) for c in (0, 1, 2, 3, 4, 5, 1024)] == [0, 1, 1, 3, 4, 1, 1]
    items = lambda rows, c, ld, dtype=1: q('yolo2_image_summary_items', rows, c, ld, dtype)      # noqa: E731
    # 256 threads x (64 / c clamped to 1 .. 16) pixels per work item
    assert [items(r, 1, 1) for r in (0, 1, 4096, 4097)] == [0, 1, 1, 2]
    assert items(104 * 104, 64, 64) == 43 and items(256, 1024, 1024) == 1 and items(257, 40, 48) == 2 and items(512, 32, 32) == 1
    assert items(4, 9, 8) == 0 and items(4, 8, 8, 2) == 0 and items(-1, 8, 8) == 0 and items(1 << 31, 1, 1) == 0      # malformed: owns nothing
    assert q('yolo2_image_summary_workspace_bytes', 3, 100) == 3 * 32 + 400 and q('yolo2_image_summary_result_bytes', 3, 100) == 3 * 16 + 100
    assert q('yolo2_image_summary_workspace_bytes', 0, 0) == 0
    with pytest.raises(_lib.HipKernelError, match='argument check failed'):
        _lib.call('yolo2_image_summary', None, 1, 0, None, 0, None, 0, None)
