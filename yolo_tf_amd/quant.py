"""Post-training int8 inference (arithmetic specified by tests/quant_ref.py).

``calibrate`` runs the bf16 engine over calibration batches and turns the abs-max of every tensor the int8 network stores into per-tensor
scales; ``QuantEngine`` walks the same graph as ``engine.Engine`` with int8 activations and host-quantised filters.  The image layer stays
on the bf16 kernels (3 input channels are no multiple of 16); its pooled output is quantised and everything behind it, the head included, runs
on yolo2_conv2d_i8.  The head writes bf16 logits, so decode, NMS and the evaluators are untouched.

Symmetric int8 in -127 .. 127: q = clip(rint(x * inv_s), -127, 127), inv_s = float32(1) / s.  Activations: one scale per tensor,
s = absmax / 127; tensors connected by a pool, reorg or concat share the max of their abs-max (those ops then move bytes).  Weights: one
scale per output channel over the BN-folded f32 filter, quantised here on the host once per set of variables.

Calibration methods: 'absmax' as above, or a clipping threshold T in the abs-max's place (s = T / 127), chosen per scale class from a
2048-bin histogram of |x| that a second pass over the batches fills on the device: 'percentile', 'mse', 'entropy' (threshold_* below).
"""
import logging
import os

import numpy as np
import torch

from . import graph as G
from . import ops
from .engine import BN_EPS, LEAKY_ALPHA, Engine

F32 = np.float32


def scale_of(amax):
    a = F32(amax)
    if not np.isfinite(a) or a == 0:
        return F32(1)
    return F32(a / F32(127))


def quantize_array(x, inv_s):
    """Host quantiser (weights): f32 array, f32 inverse scale(s) -> int8."""
    with np.errstate(invalid='ignore', over='ignore'):
        q = np.clip(np.rint(np.asarray(x, F32) * np.asarray(inv_s, F32)), F32(-127), F32(127))
    return np.where(np.isnan(q), F32(0), q).astype(np.int8)


def fold_bn(W, gamma, beta, mean, var, eps=BN_EPS):
    """W' = W * gamma / sqrt(var + eps), bias' = beta - mean * gamma / sqrt(var + eps), in f32 (what yolo2_bn_fold computes on the device)."""
    s = (np.asarray(gamma, F32) / np.sqrt(np.asarray(var, F32) + F32(eps))).astype(F32)
    return (np.asarray(W, F32) * s).astype(F32), (np.asarray(beta, F32) - np.asarray(mean, F32) * s).astype(F32)


def quantize_weights(Wf):
    """HWIO f32 -> (int8 HWIO, per-output-channel scales f32)."""
    Wf = np.asarray(Wf, F32)
    am = np.abs(Wf).reshape(-1, Wf.shape[-1]).max(axis=0)
    s = np.array([scale_of(a) for a in am], F32)
    return quantize_array(Wf, (F32(1) / s).astype(F32)), s


CALIBRATION_FILE = 'calibration.npz'      # default name, beside the checkpoints in the run's logdir


def calibration_path(logdir, path=None):
    """The calibration file of a run: ``path`` if given, else <logdir>/calibration.npz.  Exits with a message when there is none."""
    path = os.path.expanduser(os.path.expandvars(path)) if path else os.path.join(logdir, CALIBRATION_FILE)
    if not os.path.isfile(path):
        raise SystemExit('no calibration file %s: --dtype int8 needs the scales of this checkpoint -- run quantize.py first '
                         '(python quantize.py -c <the same config files> -o %s)' % (path, path))
    return path


class QuantPlan(object):
    """Which tensors of a graph are stored as int8 and which of them share a scale.

    Supported: the YOLOv2 graphs -- a batch-normalised image convolution followed by a stride-2 pool (bf16), then convolutions whose input
    channel count is a multiple of 16, pools, reorg and concat, ending in the linear head."""

    def __init__(self, graph):
        ops_ = graph.ops
        if any(op['kind'] in ('flatten', 'dropout') or op.get('fc') or (op['kind'] == 'conv' and not op['bn'] and op['act']) for op in ops_):
            raise NotImplementedError('int8 inference covers the YOLOv2 family: the YOLO (v1) fully connected head is not quantised')
        inputs = set(graph.inputs.values())
        if (len(ops_) < 3 or ops_[0]['kind'] != 'conv' or ops_[0]['x'] not in inputs or not ops_[0]['bn'] or ops_[1]['kind'] != 'pool'
                or ops_[1]['x'] is not ops_[0]['out'] or ops_[1]['stride'] != 2):
            raise NotImplementedError('int8 inference expects an image convolution followed by a stride-2 pool')
        self.first_conv, self.first_pool = ops_[0], ops_[1]
        self.body = ops_[2:]
        q = []
        for op in self.body:
            if op['kind'] == 'conv':
                if op['cin'] % 16 != 0 or op['x'] in inputs:
                    raise NotImplementedError('%s: %d input channels are not a multiple of 16' % (op['name'], op['cin']))
                if op is not ops_[-1] and not op['bn']:
                    raise NotImplementedError('%s: only the last layer may be linear' % op['name'])
            elif op['kind'] not in ('pool', 'reorg', 'concat'):
                raise NotImplementedError('int8 inference: op %s' % op['kind'])
            for t in (op.get('inputs') or [op['x']]) + [op['out']]:
                if t not in q and not (op is ops_[-1] and t is op['out']):
                    q.append(t)
        if ops_[-1]['kind'] != 'conv' or ops_[-1]['bn']:
            raise NotImplementedError('int8 inference expects a linear head')
        self.tensors = q                          # int8 tensors in order of first use; the head's output stays bf16
        parent = {t: t for t in q}

        def find(t):
            while parent[t] is not t:
                t = parent[t]
            return t
        for op in self.body:
            if op['kind'] in ('pool', 'reorg', 'concat'):
                members = (op.get('inputs') or [op['x']]) + [op['out']]
                for t in members[1:]:
                    a, b = find(members[0]), find(t)
                    if a is not b:
                        parent[b] = a
        groups = {}
        for t in q:
            groups.setdefault(find(t), []).append(t)
        self.classes = list(groups.values())

    def names(self):
        return [t.name for t in self.tensors]


METHODS = ('absmax', 'percentile', 'mse', 'entropy')
BINS = 2048                 # YOLO2_CALIB_BINS: bins of a calibration histogram over [0, abs-max of the scale class]
FIRST_CANDIDATE = 128       # the smallest clipping threshold 'mse' and 'entropy' consider, in bins (one sixteenth of the abs-max)


# ---- clipping thresholds from a histogram of |x| (host, f64; specification: tests/calib_ref.py) ---------------------------------------------
# h: counts of BINS equal bins over [0, limit], values above limit in the last one; w = limit / BINS.  Each rule returns the threshold T that
# takes the abs-max's place in scale_of; candidates are bin edges T_i = i * w, the smallest i wins ties.

def threshold_percentile(h, limit, p=99.99):
    """The upper edge of the first bin at which the cumulative count reaches ceil(total * p / 100); p = 100: the limit itself."""
    h = np.asarray(h, np.int64)
    total = int(h.sum())
    if p >= 100 or total == 0:
        return float(limit)
    need = int(np.ceil(total * float(p) / 100.0))
    b = int(np.searchsorted(np.cumsum(h), need, side='left'))
    return (b + 1) * (float(limit) / BINS)


def _mse_objective(h, limit):
    """sum over bins of h_b (x_b - q_b)^2 for every candidate i = FIRST_CANDIDATE .. BINS: the project's quantiser, s = T_i / 127, applied to
    the bin centres x_b = (b + 0.5) w.  -> f64 [BINS - FIRST_CANDIDATE + 1]"""
    w = float(limit) / BINS
    x = (np.arange(BINS, dtype=np.float64) + 0.5) * w
    s = (np.arange(FIRST_CANDIDATE, BINS + 1, dtype=np.float64) * w / 127.0)[:, None]
    q = np.minimum(np.rint(x[None, :] / s), 127.0) * s
    return ((x[None, :] - q) ** 2) @ np.asarray(h, np.float64)


def threshold_mse(h, limit):
    if int(np.asarray(h, np.int64).sum()) == 0:
        return float(limit)
    return (FIRST_CANDIDATE + int(np.argmin(_mse_objective(h, limit)))) * (float(limit) / BINS)


def _kl(h, i):
    """KL(P || Q) of candidate i, or None when Q is 0 somewhere P is not.  P: the first i bins with everything above folded into bin i - 1.
    Q: those i bins (without the folded tail) merged into 128 groups by b * 128 // i, each group's sum spread evenly over its non-zero bins."""
    head = h[:i]
    P = head.copy()
    P[i - 1] += h[i:].sum()
    g = np.arange(i) * 128 // i
    nz = head > 0
    gsum = np.bincount(g, weights=head, minlength=128)
    gnz = np.bincount(g, weights=nz, minlength=128)
    Q = np.where(nz, gsum[g] / np.maximum(gnz[g], 1.0), 0.0)
    pos = P > 0
    if (Q[pos] == 0).any():
        return None
    P = P / P.sum()
    Q = Q / Q.sum()
    return float(np.sum(P[pos] * np.log(P[pos] / Q[pos])))


def threshold_entropy(h, limit):
    """The usual KL calibrator: the candidate whose 128-level picture of the clipped distribution loses the least information."""
    h = np.asarray(h, np.float64)
    best, best_i = None, BINS
    if h.sum() > 0:
        for i in range(FIRST_CANDIDATE, BINS + 1):
            kl = _kl(h, i)
            if kl is not None and (best is None or kl < best):
                best, best_i = kl, i
    return best_i * (float(limit) / BINS)


def choose_threshold(h, limit, method, percentile=99.99):
    if method == 'percentile':
        return threshold_percentile(h, limit, percentile)
    if method == 'mse':
        return threshold_mse(h, limit)
    if method == 'entropy':
        return threshold_entropy(h, limit)
    raise ValueError('calibration method %r: expected one of %s' % (method, ', '.join(METHODS)))


def histogram_sqnr_db(h, limit, T):
    """The histogram's estimate of the signal-to-quantisation-noise ratio under threshold T, in dB: bin centres through the quantiser."""
    w = float(limit) / BINS
    x = (np.arange(BINS, dtype=np.float64) + 0.5) * w
    s = float(T) / 127.0
    q = np.minimum(np.rint(x / s), 127.0) * s
    h = np.asarray(h, np.float64)
    noise, signal = float(np.sum(h * (x - q) ** 2)), float(np.sum(h * x * x))
    return 10.0 * np.log10(signal / noise) if noise > 0 and signal > 0 else float('inf')


class Calibration(object):
    """Names and f32 scales of the int8 tensors of one network (tensors of a scale class carry the same value).  A calibration made with a
    clipping method also records the method, every tensor's class abs-max and the threshold chosen for it; the int8 engine reads the scales."""

    def __init__(self, scales, method='absmax', amax=None, thresholds=None):
        self.scales = {str(k): F32(v) for k, v in scales.items()}
        self.method = str(method)
        self.amax = None if amax is None else {str(k): F32(v) for k, v in amax.items()}
        self.thresholds = None if thresholds is None else {str(k): F32(v) for k, v in thresholds.items()}

    def save(self, path):
        names = sorted(self.scales)
        arrays = dict(names=np.array(names), scales=np.array([self.scales[n] for n in names], F32))
        if self.method != 'absmax':
            arrays.update(method=np.array(self.method), amax=np.array([self.amax[n] for n in names], F32),
                          thresholds=np.array([self.thresholds[n] for n in names], F32))
        with open(path, 'wb') as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path):
        z = np.load(path, allow_pickle=False)
        names = [str(n) for n in z['names']]
        if 'method' not in z.files:
            return cls(dict(zip(names, z['scales'].astype(F32))))
        return cls(dict(zip(names, z['scales'].astype(F32))), method=str(z['method']), amax=dict(zip(names, z['amax'].astype(F32))),
                   thresholds=dict(zip(names, z['thresholds'].astype(F32))))

    def __eq__(self, other):
        return (isinstance(other, Calibration) and self.scales == other.scales and self.method == other.method and self.amax == other.amax
                and self.thresholds == other.thresholds)


def calibration_from_absmax(classes, amax):
    """classes: [[tensor name]]; amax: {tensor name: abs-max} -> Calibration with s = (the largest abs-max of the class) / 127."""
    scales = {}
    for cls in classes:
        s = scale_of(max(F32(amax[n]) for n in cls))
        for n in cls:
            scales[n] = s
    return Calibration(scales)


def calibration_from_histograms(classes, limits, hists, method, percentile=99.99):
    """classes: [[tensor name]]; limits[k] / hists[k]: the abs-max of class k and the histogram of |x| over [0, limits[k]] its members share.
    -> (Calibration, one report dict per class that has a histogram).  A class whose abs-max is 0 or not finite keeps s = 1."""
    scales, amax, thresholds, report = {}, {}, {}, []
    for cls, limit, h in zip(classes, limits, hists):
        limit = T = F32(limit)
        h = np.asarray(h, np.int64)
        if np.isfinite(limit) and limit > 0 and h.sum() > 0:
            T = F32(choose_threshold(h, limit, method, percentile))
            first = int(round(float(T) / (float(limit) / BINS)))
            report.append({'members': list(cls), 'amax': float(limit), 'threshold': float(T), 'clipped': float(h[first:].sum()) / float(h.sum()),
                           'sqnr_db': histogram_sqnr_db(h, limit, T), 'sqnr_db_absmax': histogram_sqnr_db(h, limit, limit)})
        for n in cls:
            scales[n], amax[n], thresholds[n] = scale_of(T), limit, T
    return Calibration(scales, method=method, amax=amax, thresholds=thresholds), report


class Calibrator(object):
    """Running abs-max of every int8 tensor over the batches shown to ``observe``, on the bf16 engine in inference mode.

    The session's own engine never stores the activation in front of a fused max pool, and the abs-max of a scale class is taken over the
    un-pooled tensor too, so the calibrator drives an engine of its own with the pools un-fused (the image layer's excepted: its raw output
    is not an int8 tensor).  ``engine`` is that engine: after ``observe`` its activations are the ones the abs-max was taken of.

    ``method`` 'absmax' stops there.  'percentile', 'mse' and 'entropy' need a second pass over the same batches, ``observe_histogram``: its
    first call freezes each scale class's abs-max as the range of one 2048-bin histogram of |x| shared by the class's tensors
    (yolo2_calib_histogram, one launch per batch), and ``finish`` puts the threshold the method picks from it in the abs-max's place."""

    def __init__(self, detect_session, method='absmax', percentile=99.99):
        if method not in METHODS:
            raise ValueError('calibration method %r: expected one of %s' % (method, ', '.join(METHODS)))
        if not 0 < float(percentile) <= 100:
            raise ValueError('percentile %r is not in (0, 100]' % (percentile,))
        self.method, self.percentile = method, float(percentile)
        self.hist_jobs, self.hist_batches, self.limits = None, 0, None
        src = detect_session.engine
        if not isinstance(src, Engine):
            raise TypeError('calibration runs on a bf16 / f32 DetectSession')
        self.plan = QuantPlan(src.graph)
        self.engine = e = Engine(src.graph, src.B, 'bf16', training=False, device=src.device, pools='image')
        e.set_variables(src.get_variables())
        jobs = []
        for i, t in enumerate(self.plan.tensors):
            buf, ld = e.act[t]
            jobs.append((buf, e.B * t.h * t.w, t.c, ld, i))
        self.jobs = ops.AbsmaxJobs(jobs, len(jobs), device=e.device)
        self.batches = 0

    def observe(self, images, preprocess_mode=0):
        """Pass 1.  images: device f32 [B,H,W,3] as for DetectSession.run."""
        if self.limits is not None:
            raise RuntimeError('the histogram ranges are frozen: observe() cannot follow observe_histogram()')
        self.engine.set_images(images, preprocess_mode)
        self.engine.forward()
        self.jobs.launch()
        self.batches += 1

    def absmax(self):
        """-> ({tensor name: abs-max f32}, total number of non-finite values met)"""
        amax, bad = self.jobs.result()
        return {t.name: F32(a) for t, a in zip(self.plan.tensors, amax)}, int(bad.sum())

    def class_absmax(self):
        """-> [abs-max f32 of each scale class, in the order of plan.classes]"""
        amax, _ = self.absmax()
        return [F32(max(amax[t.name] for t in cls)) for cls in self.plan.classes]

    def observe_histogram(self, images, preprocess_mode=0):
        """Pass 2 (the clipping methods): the same batches again, after every observe().  The first call freezes the ranges."""
        if self.method == 'absmax':
            raise RuntimeError("method 'absmax' takes no histogram")
        if self.limits is None:
            assert self.batches > 0, 'no calibration batch was observed'
            self.limits = self.class_absmax()
            e, jobs = self.engine, []
            for k, (cls, limit) in enumerate(zip(self.plan.classes, self.limits)):
                if not np.isfinite(limit) or limit == 0:      # nothing to bin: the class keeps s = 1
                    continue
                for t in cls:
                    buf, ld = e.act[t]
                    jobs.append((buf, e.B * t.h * t.w, t.c, ld, k, limit))
            if jobs:
                self.hist_jobs = ops.CalibHistogramJobs(jobs, len(self.plan.classes), device=e.device)
        self.engine.set_images(images, preprocess_mode)
        self.engine.forward()
        if self.hist_jobs is not None:
            self.hist_jobs.launch()
        self.hist_batches += 1

    def histograms(self):
        """-> (counts int64 [classes, 2048], values above the frozen range int64 [classes]); zeros for a class without a job"""
        n = len(self.plan.classes)
        if self.hist_jobs is None:
            return np.zeros((n, BINS), np.int64), np.zeros(n, np.int64)
        h, _, clamped = self.hist_jobs.result()
        return h, clamped

    def finish(self):
        assert self.batches > 0, 'no calibration batch was observed'
        amax, bad = self.absmax()
        if bad:
            logging.warning('calibration: %d non-finite activation values were ignored', bad)
        classes = [[t.name for t in cls] for cls in self.plan.classes]
        if self.method == 'absmax':
            return calibration_from_absmax(classes, amax)
        if self.hist_batches == 0:
            raise RuntimeError("calibration method '%s' needs a second pass over the calibration batches: call observe_histogram() for each of "
                               'them after the last observe()' % self.method)
        h, clamped = self.histograms()
        if clamped.sum():
            logging.warning('calibration: %d values lay above the abs-max of the first pass and were counted in the last bin (the second pass '
                            'saw other data than the first)', int(clamped.sum()))
        calibration, self.report = calibration_from_histograms(classes, self.limits, h, self.method, self.percentile)
        return calibration


def calibrate(detect_session, batches, preprocess_mode=0, method='absmax', percentile=99.99):
    """batches: iterable of device f32 image tensors [B,H,W,3] -> Calibration.  The clipping methods go over the batches twice (a one-shot
    iterator is materialised into a list first)."""
    c = Calibrator(detect_session, method, percentile)
    if method != 'absmax' and iter(batches) is batches:
        batches = list(batches)
    for images in batches:
        c.observe(images, preprocess_mode)
    if method != 'absmax':
        for images in batches:
            c.observe_histogram(images, preprocess_mode)
    return c.finish()


class QuantEngine(object):
    """Inference engine with int8 activations: the surface of ``Engine`` that inference uses (set_images, forward, act, output, device,
    get_variables / set_variables).  Filters are re-quantised on the next forward after the variables change."""

    def __init__(self, graph, batch_size, calibration, seed=0, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError('yolo_tf_amd.QuantEngine needs an MI355X (no CPU path exists)')
        ops._lib.load()
        self.plan = p = QuantPlan(graph)
        missing = [n for n in p.names() if n not in calibration.scales]
        if missing:
            raise ValueError('the calibration does not cover this network: no scale for %s' % ', '.join(missing[:4]))
        self.graph, self.B, self.training, self.dtype = graph, int(batch_size), False, torch.bfloat16
        self.calibration = calibration
        self.device = dev = torch.device(device if device is not None else 'cuda:%d' % torch.cuda.current_device())
        # the image layer and its pool: a bf16 engine over that two-op graph
        (inp,) = graph.inputs.values()
        c0 = p.first_conv
        g0 = G.Graph()
        img = G.placeholder(g0, inp.name, inp.h, inp.w)
        y0 = G.conv2d(img, c0['cout'], c0['ksize'], scope=c0['name'], center=c0['beta'].name.endswith('BatchNorm/beta'),
                      weights_initializer=c0['weights'].init)
        self._pool0 = G.max_pool2d(y0, 2, scope=p.first_pool['name'])
        self.first = Engine(g0, self.B, 'bf16', training=False, seed=seed, device=dev)
        # int8 activations (a byte per element, the graph's strides and concat offsets) and the bf16 logits
        roots, self.act = {}, {}
        out = graph.ops[-1]['out']
        for t in p.tensors + [out]:
            r, off, ld = t.storage()
            if r.name not in roots:
                roots[r.name] = torch.zeros(self.B * r.h * r.w * r.ld, dtype=torch.bfloat16 if t is out else torch.int8, device=dev)
            self.act[t] = (roots[r.name][off:], ld)
        self._roots = roots
        self.scale = {t: F32(calibration.scales[t.name]) for t in p.tensors}
        self.conv = {}
        self._values = {}
        self.init_variables(seed)

    # ---------------------------------------------------------------- variables (host masters)
    def init_variables(self, seed=0):
        rng = np.random.RandomState(seed)
        for v in self.graph.variables.values():
            self._values[v.name] = v.init(rng, v.shape)
        self._dirty = True

    def get_variables(self):
        return {k: v.copy() for k, v in self._values.items()}

    def set_variables(self, values, strict=True):
        for v in self.graph.variables.values():
            if v.name in values:
                a = np.asarray(values[v.name], F32)
                assert a.shape == v.shape, (v.name, a.shape, v.shape)
                self._values[v.name] = np.ascontiguousarray(a)
            elif strict:
                raise KeyError(v.name)
        self._dirty = True

    def _prepare(self):
        if not self._dirty:
            return
        val, dev = self._values, self.device
        self.first.set_variables({v.name: val[v.name] for v in self.first.graph.variables.values()})
        for op in self.plan.body:
            if op['kind'] != 'conv':
                continue
            if op['bn']:
                Wf, bias = fold_bn(val[op['weights'].name], val[op['gamma'].name], val[op['beta'].name], val[op['moving_mean'].name],
                                   val[op['moving_variance'].name])
            else:
                Wf, bias = val[op['weights'].name], val[op['biases'].name]
            wq, s_w = quantize_weights(Wf)
            k, cin, cout = op['ksize'], op['cin'], op['cout']
            fq = np.ascontiguousarray(wq.reshape(k * k, cin, cout).transpose(2, 0, 1))       # the kernel's layout: [filter][tap][channel]
            mult = (self.scale[op['x']] * s_w).astype(F32)
            self.conv[op['name']] = {'F': torch.from_numpy(fq.reshape(-1)).to(dev), 'mult': torch.from_numpy(mult).to(dev),
                                     'bias': torch.from_numpy(np.ascontiguousarray(bias, F32)).to(dev), 's_w': s_w}
        self._dirty = False

    # ---------------------------------------------------------------- inference
    def set_images(self, images, mode=0):
        self.first.set_images(images, mode)

    def output(self):
        return self.graph.ops[-1]['out']

    def forward(self):
        self._prepare()
        B, p = self.B, self.plan
        self.first.forward()
        t0 = p.first_pool['out']
        src, lds = self.first.act[self._pool0]
        dst, ldd = self.act[t0]
        ops.quantize(src, lds, dst, ldd, B * t0.h * t0.w, t0.c, F32(1) / self.scale[t0])
        last = self.graph.ops[-1]
        for op in p.body:
            kind = op['kind']
            if kind == 'conv':
                x, out = op['x'], op['out']
                xb, ldx = self.act[x]
                ob, ldo = self.act[out]
                st = self.conv[op['name']]
                if op is last:
                    ops.conv2d_i8(xb, st['F'], st['mult'], st['bias'], ob, B, x.h, x.w, x.c, ldx, op['cout'], ldo, op['ksize'], 1.0, 1.0, ops.I8_OUT_BF16)
                else:
                    ops.conv2d_i8(xb, st['F'], st['mult'], st['bias'], ob, B, x.h, x.w, x.c, ldx, op['cout'], ldo, op['ksize'], LEAKY_ALPHA,
                                  F32(1) / self.scale[out], ops.I8_OUT_I8)
            elif kind == 'pool':
                x, out = op['x'], op['out']
                ops.maxpool_i8(self.act[x][0], self.act[x][1], self.act[out][0], self.act[out][1], B, x.h, x.w, x.c, op['stride'])
            elif kind == 'reorg':
                x, out = op['x'], op['out']
                assert self.act[x][1] == x.c
                ops.reorg_i8(self.act[x][0], self.act[out][0], B, x.h, x.w, x.c, self.act[out][1])
