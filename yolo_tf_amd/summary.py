"""Histogram summaries: the reference's ``[summary] histogram`` and ``gradients`` keys (train.py:56-61 there, slim's
``summarize_gradients``), binned on the device by yolo2_histogram (csrc/summary.hip).

The reference applies ``re.match`` of the pattern to every op name of its TF graph (utils.match_tensor) and hands the matches to
``tf.summary.histogram``.  This graph has no ops to enumerate; the names that can be summarised are

  * every variable, trainable or not (``<scope>/weights``, ``.../BatchNorm/gamma``, ``.../BatchNorm/moving_mean`` ...),
  * the batch moments of every normalised layer under the names slim's batch_norm gives them,
    ``<scope>/BatchNorm/moments/normalize/mean`` and ``.../variance`` (the engine's ``conv[...]['mean' | 'var']``),
  * the activations the training forward stores (Engine.summarizable_tensors), spelled as the reference's graph spells them:
    ``<scope>/convolution``, ``<scope>/leaky_relu/data`` for this graph's ``<scope>/leaky_relu``, ``<model scope>/input`` for the image
    tensor after standardisation; pooling, reorg, concat and BiasAdd outputs keep their names.

A pattern that matches only tensors the forward never stores logs one warning and summarises nothing for them, as the reference
warns about a disabled summary.  ``gradients = 1`` adds, for every trainable variable, the histogram ``<var>/gradient`` and the scalar
``<var>/gradient_norm`` = sqrt(sum of squares) of the gradient arena as the optimizer consumed it: after the all-reduce (the SUM over
replicas when nothing is clipped -- the update applies the 1 / world factor itself) and after clipping.  (slim/learning.py
add_gradients_summaries is restated from memory: DESIGN.md.)

A missing section or key means disabled -- the reference's default config spells the key ``histogram_``, which disables it the same
way -- and then nothing is allocated and nothing is launched.

Image summaries: the reference's ``[summary] image`` and ``image_max`` keys (train.py:44-53 there) select activations by the same names and
hand them to ``tf.summary.image``; here yolo2_image_summary (csrc/image_summary.hip) makes the bytes of the first ``image_max`` images of
every matched, stored activation on the device (ImageSummaries below), and utils/png.py wraps them."""
import logging
import math
import re

import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
MOMENTS = (('mean', 'BatchNorm/moments/normalize/mean'), ('var', 'BatchNorm/moments/normalize/variance'))


def _limits():
    pos, v = [], 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    return np.array([-p for p in reversed(pos)] + [0.0] + pos + [DBL_MAX], np.float64)


LIMITS = _limits()


def encode_buckets(counts):
    """HistogramProto's (bucket_limit, bucket) of 1550 counts, as TensorFlow's EncodeToProto(preserve_zero_buckets = false): a run of empty
    buckets becomes one entry with the run's last limit and count 0, every non-empty bucket keeps its own limit."""
    counts = np.asarray(counts)
    assert counts.shape == LIMITS.shape
    filled = counts > 0
    # an entry ends at bucket i when i is non-empty, or when i is empty and the next bucket is not (or there is none)
    ends = filled | np.append(filled[1:], True)
    idx = np.nonzero(ends)[0]
    return [float(v) for v in LIMITS[idx]], [float(v) for v in np.where(filled[idx], counts[idx], 0)]


def activation_tag(name, model_scope, is_input=False):
    if is_input:
        return model_scope + '/input'
    if name.endswith('/leaky_relu'):
        return name + '/data'
    return name


def summarizable_names(graph):
    """Every name a ``[summary] histogram`` pattern is matched against, from the graph alone (no device): [(tag, kind, key)] with kind
    'variable' (key: variable name), 'moment' (key: (op name, 'mean' | 'var')) or 'activation' (key: graph Tensor).  Whether an activation is
    stored is the engine's knowledge (Engine.summarizable_tensors)."""
    scope = next(iter(graph.variables)).split('/')[0]
    names = [(v.name, 'variable', v.name) for v in graph.variables.values()]
    for op in graph.ops:
        if op['kind'] == 'conv' and op['bn']:
            names += [('%s/%s' % (op['name'], tag), 'moment', (op['name'], key)) for key, tag in MOMENTS]
    inputs = set(graph.inputs.values())
    for t in graph.tensors:
        if t.flat_of is None:
            names.append((activation_tag(t.name, scope, t in inputs), 'activation', t))
    return names


def read_config(config):
    """-> (histogram pattern or None, gradients flag) from the reference's own keys."""
    pattern, gradients = None, False
    if config is not None and config.has_section('summary'):
        if config.has_option('summary', 'histogram'):
            pattern = config.get('summary', 'histogram').strip() or None
        if config.has_option('summary', 'gradients'):
            gradients = config.getint('summary', 'gradients') != 0
    return pattern, gradients


class HistogramSummaries(object):
    def __init__(self, session, config):
        self.session = session
        self.pattern, self.gradients = read_config(config)
        self.enabled = self.pattern is not None or self.gradients
        self._plans = {}           # bound input size -> (tags, ops.HistogramJobs, pinned host buffer)
        self._pending = None
        self._warned = set()

    def resolve(self, graph=None):
        """-> [(tag, kind, key)] selected by the pattern and the gradients flag, in graph order (pure host logic)."""
        graph = graph if graph is not None else self.session.engine.graph
        prog = re.compile(self.pattern) if self.pattern is not None else None
        picked = [n for n in summarizable_names(graph) if prog is not None and prog.match(n[0])]
        if self.gradients:
            picked += [(v.name + '/gradient', 'gradient', v.name) for v in graph.trainable()]
        return picked

    def _plan(self):
        from . import ops
        e = self.session.engine
        key = id(e._cur)
        if key in self._plans:
            return self._plans[key]
        import torch
        stored = dict((t, where) for t, where in e.summarizable_tensors())
        tags, jobs, missing = [], [], []
        for tag, kind, ref in self.resolve(e.graph):
            if kind == 'variable':
                t = e.var[ref]
                job = (t, 1, t.numel(), t.numel())
            elif kind == 'gradient':
                t = e.gvar[ref]
                job = (t, 1, t.numel(), t.numel())
            elif kind == 'moment':
                t = e.conv[ref[0]][ref[1]]
                job = (t, 1, t.numel(), t.numel())
            else:
                if stored.get(ref) is None:
                    missing.append(tag)
                    continue
                job = stored[ref]
            tags.append(tag)
            jobs.append(job)
        if missing and 'missing' not in self._warned:
            self._warned.add('missing')
            logging.warning('[summary] histogram: %d matched tensor(s) are never stored by the training forward and are skipped: %s',
                            len(missing), ', '.join(missing[:8]) + (' ...' if len(missing) > 8 else ''))
        if not jobs:
            if 'empty' not in self._warned:
                self._warned.add('empty')
                logging.warning('[summary] histogram = %r selects nothing that can be summarised: histogram summaries disabled', self.pattern)
            plan = (tags, None, None)
        else:
            table = ops.HistogramJobs(jobs, device=e.device)
            host = torch.empty(table.out.shape, dtype=torch.int64).pin_memory()
            plan = (tags, table, host)
        self._plans[key] = plan
        return plan

    def collect(self):
        """Enqueues the binning call and ONE asynchronous copy of the records to pinned host memory on the current stream; no
        synchronisation.  Call it after a step, before the next one overwrites the gradients and activations."""
        if not self.enabled:
            return
        import torch
        tags, table, host = self._plan()
        if table is None:
            return
        table.launch()
        host.copy_(table.out, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self._pending = (tags, host, done)

    def results(self):
        """Waits for the last collect() and returns (histograms [(tag, record)], scalars [(tag, value)]); record: ops.decode_histograms."""
        from . import ops
        if self._pending is None:
            return [], []
        tags, host, done = self._pending
        self._pending = None
        done.synchronize()
        records = ops.decode_histograms(host.numpy().copy())       # (a copy: the pinned buffer is the next collection's destination)
        scalars = [(tag[:-len('/gradient')] + '/gradient_norm', math.sqrt(r['sum_squares'])) for tag, r in zip(tags, records) if tag.endswith('/gradient')] \
            if self.gradients else []
        return list(zip(tags, records)), scalars

    def write(self, writer, step):
        """Encodes the collected records and appends them (and the gradient norms) to ``writer`` as one event of ``step``."""
        histograms, scalars = self.results()
        if not histograms:
            return 0
        protos = []
        for tag, r in histograms:
            if r['nonfinite']:
                logging.warning('histogram summary %s: %d NaN / Inf value(s) left out (TensorFlow would have aborted the summary)', tag, r['nonfinite'])
            limit, bucket = encode_buckets(r['counts'])
            protos.append((tag, {'min': r['min'], 'max': r['max'], 'num': float(r['num']), 'sum': r['sum'], 'sum_squares': r['sum_squares'],
                                 'bucket_limit': limit, 'bucket': bucket}))
        writer.add_histograms(step, protos, scalars=scalars or None)
        return len(protos)


def read_image_config(config):
    """-> (image pattern, image_max) from the reference's own keys, or (None, None) when either is missing: the reference's summary_image
    catches NoSectionError / NoOptionError of both ``config.get('summary', 'image')`` and ``config.getint('summary', 'image_max')``."""
    if config is None or not config.has_section('summary') or not config.has_option('summary', 'image'):
        return None, None
    pattern = config.get('summary', 'image').strip() or None
    if pattern is None or not config.has_option('summary', 'image_max'):
        return None, None
    image_max = config.getint('summary', 'image_max')
    if image_max < 1:
        raise ValueError('[summary] image_max = %d: tf.summary.image needs max_outputs >= 1' % image_max)
    return pattern, image_max


def image_tags(name, image_max, batch):
    """tf.summary.image's tags: ``<name>/image`` when max_outputs is 1, otherwise ``<name>/image/<i>`` for the first min(max_outputs, batch)."""
    return [name + '/image'] if image_max == 1 else ['%s/image/%d' % (name, i) for i in range(min(image_max, batch))]


class ImageSummaries(object):
    def __init__(self, session, config):
        self.session = session
        self.pattern, self.image_max = read_image_config(config)
        self.enabled = self.pattern is not None
        if not self.enabled:
            logging.warning('summary_image disabled')         # (the reference's words for a missing section or key)
        self._plans = {}           # bound input size -> (meta [(tag, h, w, depth)], ops.ImageJobs, pinned host buffer)
        self._pending = None
        self._warned = set()
        self.records = []          # [(tag, record)] of the last results(): image_min, image_max, scale, non-finite pixels

    def resolve(self, graph=None):
        """-> [(name, graph Tensor)] of the activations the pattern selects, in graph order (pure host logic).  Variables and batch moments the
        pattern also matches are not images here: one warning, then skipped."""
        if not self.enabled:
            return []
        graph = graph if graph is not None else self.session.engine.graph
        prog = re.compile(self.pattern)
        matched = [n for n in summarizable_names(graph) if prog.match(n[0])]
        others = [tag for tag, kind, _ in matched if kind != 'activation']
        if others and 'others' not in self._warned:
            self._warned.add('others')
            logging.warning('[summary] image: %d matched variable(s) / batch moment(s) are not images and are skipped: %s',
                            len(others), ', '.join(others[:8]) + (' ...' if len(others) > 8 else ''))
        return [(tag, ref) for tag, kind, ref in matched if kind == 'activation']

    def _plan(self):
        from . import ops
        e = self.session.engine
        key = id(e._cur)
        if key in self._plans:
            return self._plans[key]
        import torch
        stored = dict((t, where) for t, where in e.summarizable_tensors())
        meta, jobs, missing = [], [], []
        for name, t in self.resolve(e.graph):
            if stored.get(t) is None:
                missing.append(name)
                continue
            buf, rows, c, ld = stored[t]
            batch, pixels = rows // (t.h * t.w), t.h * t.w
            assert batch * pixels == rows and c == t.c, (name, rows, t.h, t.w, c)
            for i, tag in enumerate(image_tags(name, self.image_max, batch)):
                meta.append((tag, t.h, t.w, ops.image_depth(c)))
                jobs.append((buf[i * pixels * ld:], pixels, c, ld))
        if missing and 'missing' not in self._warned:
            self._warned.add('missing')
            logging.warning('[summary] image: %d matched tensor(s) are never stored by the training forward and are skipped: %s',
                            len(missing), ', '.join(missing[:8]) + (' ...' if len(missing) > 8 else ''))
        if not jobs:
            if 'empty' not in self._warned:
                self._warned.add('empty')
                logging.warning('[summary] image = %r selects nothing that can be summarised: image summaries disabled', self.pattern)
            plan = (meta, None, None)
        else:
            table = ops.ImageJobs(jobs, device=e.device)
            host = torch.empty(table.out.shape, dtype=torch.uint8).pin_memory()
            plan = (meta, table, host)
        self._plans[key] = plan
        return plan

    def collect(self):
        """Enqueues the call and ONE asynchronous copy of records and bytes to pinned host memory on the current stream; no synchronisation.
        Call it after a step, before the next one overwrites the activations."""
        if not self.enabled:
            return
        import torch
        meta, table, host = self._plan()
        if table is None:
            return
        table.launch()
        host.copy_(table.out, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self._pending = (meta, table, host, done)

    def results(self):
        """Waits for the last collect() and returns [(tag, height, width, depth, uint8 array [height][width][depth])]."""
        from . import ops
        if self._pending is None:
            return []
        meta, table, host, done = self._pending
        self._pending = None
        done.synchronize()
        decoded = ops.decode_images(host.numpy().copy(), table.shapes, table.offsets)      # (a copy: the pinned buffer is the next collection's destination)
        self.records = [(m[0], rec) for m, (rec, _) in zip(meta, decoded)]
        return [(tag, h, w, depth, pix.reshape(h, w, depth)) for (tag, h, w, depth), (_, pix) in zip(meta, decoded)]

    def write(self, writer, step):
        """PNG-encodes the collected images and appends them to ``writer`` as one event of ``step``."""
        from .utils import png
        images = self.results()
        if not images:
            return 0
        for tag, rec in self.records:
            if rec['nonfinite']:
                logging.warning('image summary %s: %d pixel(s) with NaN / Inf drawn in the bad colour', tag, rec['nonfinite'])
        writer.add_images(step, [(tag, {'height': h, 'width': w, 'colorspace': depth, 'encoded_image_string': png.encode(pix)})
                                 for tag, h, w, depth, pix in images])
        return len(images)
