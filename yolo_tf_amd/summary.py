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
way -- and then nothing is allocated and nothing is launched."""
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
