"""TensorBoard event files without TensorFlow.

The reference hands ``slim.learning.train`` a ``tf.summary.FileWriter(os.path.join(logdir, args.logname))`` (train.py:141-145)
and summarises the scalars its ``[summary] scalar`` pattern selects (config.ini:63, train.py:31-41): ``total_loss`` and
``total_loss/objectives/{iou_best,iou_normal,coords,prob}``.  This module writes the same kind of file -- TFRecord framing
(utils/tfrecord.py) around serialized ``tensorflow.Event`` protos -- for exactly those scalars, hand-rolling the few tiny
messages it needs:

    Event   { double wall_time = 1; int64 step = 2; oneof { string file_version = 3; Summary summary = 5; } }
    Summary { repeated Value value = 1; }      Value { string tag = 1; float simple_value = 2; Image image = 4; HistogramProto histo = 5; }
    Image { int32 height = 1; int32 width = 2; int32 colorspace = 3; bytes encoded_image_string = 4; }
    HistogramProto { double min = 1, max = 2, num = 3, sum = 4, sum_squares = 5; repeated double bucket_limit = 6 [packed], bucket = 7 [packed]; }

TensorBoard reads it like any ``events.out.tfevents.*`` file.  Histogram summaries (train.py:56-61 of the reference, ``[summary] histogram``
and ``gradients``) and image summaries (train.py:44-53, ``[summary] image`` and ``image_max``) come from yolo_tf_amd/summary.py; the images
are PNGs written by utils/png.py.  Host-side I/O only."""
import os
import socket
import struct
import time

from . import tfrecord

SCALAR_TAGS = ('total_loss', 'total_loss/objectives/iou_best', 'total_loss/objectives/iou_normal', 'total_loss/objectives/coords',
               'total_loss/objectives/prob')


def _varint(n):
    out = bytearray()
    n &= (1 << 64) - 1
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _ld(field, payload):          # length-delimited field
    return _varint((field << 3) | 2) + _varint(len(payload)) + payload


def encode_histogram(h):
    """HistogramProto bytes of ``h``: a dict with min, max, num, sum, sum_squares and the already collapsed bucket_limit / bucket lists
    (summary.encode_buckets).  proto3 rules: a scalar field equal to zero is not written; the repeated doubles are packed."""
    out = b''
    for field, key in ((1, 'min'), (2, 'max'), (3, 'num'), (4, 'sum'), (5, 'sum_squares')):
        bits = struct.pack('<d', float(h[key]))
        if bits != b'\0' * 8:
            out += _varint((field << 3) | 1) + bits
    for field, key in ((6, 'bucket_limit'), (7, 'bucket')):
        if len(h[key]):
            out += _ld(field, struct.pack('<%dd' % len(h[key]), *[float(v) for v in h[key]]))
    return out


def decode_histogram(buf):
    out = {'min': 0.0, 'max': 0.0, 'num': 0.0, 'sum': 0.0, 'sum_squares': 0.0, 'bucket_limit': [], 'bucket': []}
    keys = {1: 'min', 2: 'max', 3: 'num', 4: 'sum', 5: 'sum_squares', 6: 'bucket_limit', 7: 'bucket'}
    i = 0
    while i < len(buf):
        key, i = _read_varint(buf, i)
        f, wt = key >> 3, key & 7
        if wt == 1:
            v, i = struct.unpack('<d', buf[i:i + 8])[0], i + 8
            if f in (6, 7):
                out[keys[f]].append(v)         # (an unpacked repeated double: legal on the wire)
            elif f in keys:
                out[keys[f]] = v
        elif wt == 2:
            n, i = _read_varint(buf, i)
            if f in (6, 7):
                out[keys[f]] += list(struct.unpack('<%dd' % (n // 8), buf[i:i + n]))
            i += n
        else:
            raise ValueError('wire type %d in a HistogramProto' % wt)
    return out


def encode_image(im):
    """Summary.Image bytes of ``im``: a dict with height, width, colorspace (the channel count: 1 grey, 3 RGB, 4 RGBA) and
    encoded_image_string (PNG bytes).  proto3 rules: a field equal to zero / empty is not written."""
    out = b''
    for field, key in ((1, 'height'), (2, 'width'), (3, 'colorspace')):
        if int(im[key]) != 0:
            out += _varint((field << 3) | 0) + _varint(int(im[key]))
    if len(im['encoded_image_string']):
        out += _ld(4, bytes(im['encoded_image_string']))
    return out


def decode_image(buf):
    out = {'height': 0, 'width': 0, 'colorspace': 0, 'encoded_image_string': b''}
    keys = {1: 'height', 2: 'width', 3: 'colorspace'}
    i = 0
    while i < len(buf):
        key, i = _read_varint(buf, i)
        f, wt = key >> 3, key & 7
        if wt == 0:
            v, i = _read_varint(buf, i)
            if f in keys:
                out[keys[f]] = v
        elif wt == 2:
            n, i = _read_varint(buf, i)
            if f == 4:
                out['encoded_image_string'] = bytes(buf[i:i + n])
            i += n
        else:
            raise ValueError('wire type %d in a Summary.Image' % wt)
    return out


def encode_event(wall_time, step=None, file_version=None, scalars=None, histograms=None, images=None):
    """``histograms``: [(tag, dict for encode_histogram)], written after the scalars into the same Summary; ``images``: [(tag, dict for
    encode_image)], written after the histograms.  None (or empty with no scalars) leaves the bytes of a scalar-only event exactly as they
    were."""
    ev = _varint((1 << 3) | 1) + struct.pack('<d', float(wall_time))
    if step is not None and step != 0:
        ev += _varint((2 << 3) | 0) + _varint(int(step))
    if file_version is not None:
        ev += _ld(3, file_version.encode())
    if scalars is not None or histograms or images:
        summary = b''
        for tag, value in (scalars or ()):
            summary += _ld(1, _ld(1, tag.encode()) + _varint((2 << 3) | 5) + struct.pack('<f', float(value)))
        for tag, h in (histograms or ()):
            summary += _ld(1, _ld(1, tag.encode()) + _ld(5, encode_histogram(h)))
        for tag, im in (images or ()):
            summary += _ld(1, _ld(1, tag.encode()) + _ld(4, encode_image(im)))
        ev += _ld(5, summary)
    return ev


def decode_event(buf):
    """Inverse of :func:`encode_event` for the fields it writes (tests, and reading files back)."""
    def fields(b):
        i = 0
        while i < len(b):
            key, i = _read_varint(b, i)
            f, wt = key >> 3, key & 7
            if wt == 0:
                v, i = _read_varint(b, i)
            elif wt == 1:
                v, i = b[i:i + 8], i + 8
            elif wt == 5:
                v, i = b[i:i + 4], i + 4
            elif wt == 2:
                n, i = _read_varint(b, i)
                v, i = b[i:i + n], i + n
            else:
                raise ValueError('wire type %d' % wt)
            yield f, wt, v

    out = {'step': 0, 'scalars': [], 'histograms': [], 'images': []}
    for f, wt, v in fields(buf):
        if f == 1:
            out['wall_time'] = struct.unpack('<d', v)[0]
        elif f == 2:
            out['step'] = v
        elif f == 3:
            out['file_version'] = v.decode()
        elif f == 5:
            for f2, _, val in fields(v):
                if f2 == 1:
                    tag, simple, histo, image = None, None, None, None
                    for f3, _, x in fields(val):
                        if f3 == 1:
                            tag = x.decode()
                        elif f3 == 2:
                            simple = struct.unpack('<f', x)[0]
                        elif f3 == 4:
                            image = decode_image(x)
                        elif f3 == 5:
                            histo = decode_histogram(x)
                    if histo is not None:
                        out['histograms'].append((tag, histo))
                    elif image is not None:
                        out['images'].append((tag, image))
                    else:
                        out['scalars'].append((tag, simple))
    return out


def _read_varint(b, i):
    shift, n = 0, 0
    while True:
        c = b[i]
        i += 1
        n |= (c & 0x7F) << shift
        if not c & 0x80:
            return n, i
        shift += 7


class FileWriter(object):
    """``tf.summary.FileWriter(logdir)`` for scalar summaries: appends to ``<logdir>/events.out.tfevents.<time>.<host>``."""

    def __init__(self, logdir):
        os.makedirs(logdir, exist_ok=True)
        now = time.time()
        self.path = os.path.join(logdir, 'events.out.tfevents.%010d.%s' % (int(now), socket.gethostname()))
        self._f = open(self.path, 'ab')
        self._write(encode_event(now, file_version='brain.Event:2'))

    def _write(self, payload):
        head = struct.pack('<Q', len(payload))
        self._f.write(head + struct.pack('<I', tfrecord.masked_crc32c(head)) + payload + struct.pack('<I', tfrecord.masked_crc32c(payload)))

    def add_scalars(self, step, values, wall_time=None):
        """values: {tag: float} or [(tag, float)]."""
        items = list(values.items()) if isinstance(values, dict) else list(values)
        self._write(encode_event(time.time() if wall_time is None else wall_time, step=step, scalars=items))

    def add_histograms(self, step, histograms, scalars=None, wall_time=None):
        """histograms: [(tag, dict for encode_histogram)]; ``scalars`` (optional [(tag, float)]) go into the same event."""
        self._write(encode_event(time.time() if wall_time is None else wall_time, step=step, scalars=scalars, histograms=list(histograms)))

    def add_images(self, step, images, wall_time=None):
        """images: [(tag, dict for encode_image)], one event."""
        self._write(encode_event(time.time() if wall_time is None else wall_time, step=step, images=list(images)))

    def add_training_summary(self, step, fetched):
        """The five scalars of the reference's [summary] section from TrainSession.fetch()'s dict; with a teacher also the
        weighted distill term and its three unweighted parts."""
        distill = [('total_loss/distill', fetched['distill'])] + [('total_loss/distill/' + k, fetched['distill_' + k]) for k in ('objectness', 'coords', 'prob')] \
            if 'distill' in fetched else []
        self.add_scalars(step, [('total_loss', fetched['total_loss'])] +
                         [('total_loss/objectives/' + k, fetched[k]) for k in ('iou_best', 'iou_normal', 'coords', 'prob')] + distill)

    def flush(self):
        self._f.flush()

    def close(self):
        self._f.close()


def read_events(path):
    return [decode_event(p) for p in tfrecord.read_records(path)]
