"""Calibration methods on the CPU: the clipping thresholds of yolo_tf_amd.quant against the specification (tests/calib_ref.py), the stated
properties on three synthetic distributions, scale classes, the calibration file, and the accuracy of each method end to end through the
int8 specification (tests/quant_ref.py) against the f32 oracle.  No GPU anywhere."""
import numpy as np
import pytest

import calib_ref as C
import quant_ref as Q
from oracle import yolo2_ref as R

N = 2 ** 18
METHODS = ('mse', 'entropy', 'percentile')


@pytest.fixture(scope='module')
def inputs():
    """(a) uniform(-1, 1); (b) a standard normal through leaky 0.1; (c) the same with four outliers of 60.  One RandomState(0), f32."""
    rng = np.random.RandomState(0)
    a = rng.uniform(-1, 1, N).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    b = np.where(b > 0, b, b * np.float32(0.1)).astype(np.float32)
    c = b.copy()
    c[:4] = 60
    out = {}
    for k, x in (('a', a), ('b', b), ('c', c)):
        amax, bad = Q.absmax(x)
        h, nonfinite, clamped = C.abs_histogram(x, amax)
        assert bad == 0 and nonfinite == 0 and clamped == 0 and int(h.sum()) == N and h[-1] >= 1
        out[k] = {'x': x, 'amax': amax, 'h': h}
    return out


@pytest.fixture(scope='module')
def chosen(inputs):
    """The product's threshold per input and method, computed once."""
    from yolo_tf_amd import quant
    return {(k, m): quant.choose_threshold(v['h'], v['amax'], m, 99.99) for k, v in inputs.items() for m in METHODS}


def sample_rms(x, T):
    """rms error of the project's quantiser on the samples, with the scale made from threshold T."""
    s = Q.scale_of(T)
    q = Q.quantize(x, Q.inv_scale(s)).astype(np.float64) * np.float64(s)
    return float(np.sqrt(np.mean((x.astype(np.float64) - q) ** 2)))


def test_thresholds_on_the_three_distributions(inputs, chosen):
    from yolo_tf_amd import quant
    ratio = {key: T / float(inputs[key[0]]['amax']) for key, T in chosen.items()}
    for k in 'abc':
        print('input (%s): T / amax  mse %.4f  entropy %.4f  percentile 99.99 %.4f' % (k, ratio[k, 'mse'], ratio[k, 'entropy'], ratio[k, 'percentile']))
    # (a) uniform: nothing to clip.  Balancing the rounding noise s^2 / 12 against the clipping noise (A - T)^3 / 3A puts the optimum at 0.9968 A
    assert 0.99 <= ratio['a', 'mse'] <= 1
    a = inputs['a']
    assert quant.choose_threshold(a['h'], a['amax'], 'entropy') == float(a['amax'])
    assert quant.choose_threshold(a['h'], a['amax'], 'percentile', 100) == float(a['amax'])
    assert np.float32(quant.choose_threshold(a['h'], a['amax'], 'percentile', 100)) == a['amax']
    # (b) a long but regular tail: every method clips some of it, none more than half the range
    for m in METHODS:
        assert 0.5 < ratio['b', m] < 1, (m, ratio['b', m])
    # (c) four outliers at 60 own the abs-max: entropy and percentile drop them
    assert ratio['c', 'entropy'] <= 0.25 and ratio['c', 'percentile'] <= 0.25


@pytest.mark.parametrize('k', ['b', 'c'])
def test_mse_threshold_is_no_worse_than_absmax_on_the_samples(inputs, chosen, k):
    x, amax = inputs[k]['x'], inputs[k]['amax']
    got, base = sample_rms(x, chosen[k, 'mse']), sample_rms(x, amax)
    print('input (%s): rms quantisation error on the samples  mse %.5f  absmax %.5f' % (k, got, base))
    assert got <= base


def test_percentile_returns_the_exact_bin_edge():
    from yolo_tf_amd import quant
    h = np.zeros(C.BINS, np.int64)
    h[10], h[500], h[2047] = 9990, 9, 1                   # cumulative: 9990 at bin 10, 9999 at bin 500, 10000 at the last
    limit = np.float32(8.0)
    w = 8.0 / C.BINS
    for p, b in ((99.9, 10), (99.91, 500), (99.99, 500), (99.995, 2047), (50, 10)):
        assert quant.threshold_percentile(h, limit, p) == (b + 1) * w == C.percentile_threshold(h, limit, p), p
    assert quant.threshold_percentile(h, limit, 100) == 8.0
    # no lower bound of 128 bins here, unlike mse and entropy
    assert quant.threshold_percentile(h, limit, 99.9) < C.FIRST * w
    assert quant.threshold_mse(h, limit) >= C.FIRST * w and quant.threshold_entropy(h, limit) >= C.FIRST * w


@pytest.mark.parametrize('method', ['mse', 'entropy'])
@pytest.mark.parametrize('k', ['a', 'b', 'c'])
def test_product_and_specification_pick_the_same_candidate(inputs, chosen, k, method):
    """Where f64 summation order separates them (the product sums with a matrix product, the specification exactly), the specification's
    objective at the product's choice is within a relative 1e-9 of its minimum: a 2048-term f64 sum is good to about 2e-13."""
    h, amax = inputs[k]['h'], inputs[k]['amax']
    w = float(amax) / C.BINS
    obj = C.objectives(h, amax, method)
    want = C.best_candidate(obj)
    got = int(round(chosen[k, method] / w))
    assert got * w == chosen[k, method] and C.FIRST <= got <= C.BINS
    if got != want:
        assert got in obj and abs(obj[got] - obj[want]) <= 1e-9 * abs(obj[want]), (got, want, obj[got], obj[want])
    assert C.threshold(h, amax, method) == want * w


@pytest.mark.parametrize('k', ['a', 'b', 'c'])
def test_percentile_of_the_product_equals_the_specification(inputs, chosen, k):
    h, amax = inputs[k]['h'], inputs[k]['amax']
    assert chosen[k, 'percentile'] == C.percentile_threshold(h, amax, 99.99)
    for p in (50, 90, 99, 99.999, 100):
        from yolo_tf_amd import quant
        assert quant.threshold_percentile(h, amax, p) == C.percentile_threshold(h, amax, p), p


def test_abs_histogram_rule_on_edges():
    limit = np.float32(3.0)
    w = np.float32(3.0) / np.float32(C.BINS)
    x = np.array([0.0, -0.0, 1e-45, -1e-40, w, -w, 5 * w, 3.0, -3.0, 3.5, 1e30, np.nan, np.inf, -np.inf], np.float32)
    h, nonfinite, clamped = C.abs_histogram(x, limit)
    assert nonfinite == 3 and clamped == 2 and int(h.sum()) == 11
    assert h[0] == 4 and h[1] == 2 and h[5] == 1 and h[2047] == 4          # a value equal to the limit sits in the last bin, unclamped


def test_scale_classes_share_one_histogram_and_empty_classes_keep_scale_one(inputs):
    from yolo_tf_amd import quant
    b = inputs['b']
    classes = [['conv1', 'pool1'], ['dead'], ['broken'], ['conv2']]
    limits = [b['amax'], np.float32(0), np.float32(np.nan), inputs['c']['amax']]
    hists = [b['h'], np.zeros(C.BINS, np.int64), np.zeros(C.BINS, np.int64), inputs['c']['h']]
    cal, report = quant.calibration_from_histograms(classes, limits, hists, 'percentile', 99.99)
    T = np.float32(C.percentile_threshold(b['h'], b['amax'], 99.99))
    assert cal.scales['conv1'] == cal.scales['pool1'] == Q.scale_of(T) and cal.thresholds['conv1'] == cal.thresholds['pool1'] == T
    assert cal.amax['conv1'] == cal.amax['pool1'] == b['amax']
    assert cal.scales['dead'] == 1 and cal.scales['broken'] == 1
    assert cal.scales['conv2'] == Q.scale_of(np.float32(C.percentile_threshold(inputs['c']['h'], inputs['c']['amax'], 99.99)))
    assert cal.method == 'percentile' and [r['members'] for r in report] == [['conv1', 'pool1'], ['conv2']]
    r = report[0]
    assert 0 < r['clipped'] <= 1e-4 and r['threshold'] == float(T) and r['amax'] == float(b['amax'])
    # the four outliers go, with at most the 0.01 % the percentile allows: N - ceil(N * 0.9999) = 26 values
    assert 4 <= round(report[1]['clipped'] * N) <= 26
    # the abs-max is one of the candidates of 'mse', so its histogram estimate of the SQNR can only be at least as good
    for r in quant.calibration_from_histograms(classes, limits, hists, 'mse')[1]:
        assert np.isfinite(r['sqnr_db']) and r['sqnr_db'] >= r['sqnr_db_absmax']
    with pytest.raises(ValueError, match='method'):
        quant.calibration_from_histograms(classes, limits, hists, 'median')


def test_calibration_file_with_and_without_the_new_keys(tmp_path, inputs):
    from yolo_tf_amd import quant
    b = inputs['b']
    cal, _ = quant.calibration_from_histograms([['x', 'y'], ['z']], [b['amax'], np.float32(0)], [b['h'], np.zeros(C.BINS, np.int64)], 'mse')
    path = str(tmp_path / 'mse.npz')
    cal.save(path)
    z = np.load(path)
    assert sorted(z.files) == ['amax', 'method', 'names', 'scales', 'thresholds'] and str(z['method']) == 'mse'
    assert z['amax'].dtype == z['thresholds'].dtype == z['scales'].dtype == np.float32
    back = quant.Calibration.load(path)
    assert back == cal and back.method == 'mse' and back.thresholds == cal.thresholds and back.amax == cal.amax and back.scales == cal.scales
    # a file from before the methods existed: names and scales only
    old = str(tmp_path / 'old.npz')
    np.savez(old, names=np.array(['x', 'y']), scales=np.array([0.5, 0.25], np.float32))
    got = quant.Calibration.load(old)
    assert got.method == 'absmax' and got.amax is None and got.thresholds is None
    assert got == quant.Calibration({'x': np.float32(0.5), 'y': np.float32(0.25)}) and got != cal


def test_absmax_method_is_what_it_was(tmp_path):
    """calibration_from_absmax is the rule Calibrator.finish() had: the class's largest abs-max over 127, s = 1 for 0; the file has the two keys."""
    from yolo_tf_amd import quant
    nodes = Q.plan(R.darknet_spec(20, 5))
    rng = np.random.RandomState(5)
    amax = {t: np.float32(rng.rand() * 10) for t in sorted(Q.int8_tensors(nodes))}
    amax['conv3'] = np.float32(0)
    classes = [sorted(c) for c in Q.scale_classes(nodes)]
    cal = quant.calibration_from_absmax(classes, amax)
    assert cal.scales == Q.resolve_scales(nodes, amax) and cal.scales['conv3'] == 1
    assert cal == quant.Calibration(Q.resolve_scales(nodes, amax)) and cal.method == 'absmax'
    path = str(tmp_path / 'calibration.npz')
    cal.save(path)
    assert sorted(np.load(path).files) == ['names', 'scales'] and quant.Calibration.load(path) == cal
    import inspect
    assert inspect.signature(quant.Calibrator.__init__).parameters['method'].default == 'absmax'
    assert inspect.signature(quant.calibrate).parameters['method'].default == 'absmax'


def test_calib_histogram_argument_errors_raise_without_touching_the_gpu():
    from yolo_tf_amd import _lib
    ok = 1 << 20                                          # an aligned, never dereferenced address
    for args in ((None, 1, ok, None), (ok, 1, None, None), (ok, 0, ok, None), (ok, -1, ok, None), (ok, 65536, ok, None)):
        with pytest.raises(_lib.HipKernelError, match='yolo2_calib_histogram: argument check failed'):
            _lib.call('yolo2_calib_histogram', *args)


# ---- end to end: each method's thresholds through the int8 specification, against the f32 oracle ----------------------------------------------

SIZE, B = 64, 2


@pytest.fixture(scope='module')
def nets():
    from test_quant_cpu import f32_activations, seeded_params
    cache = {}

    def get(inference):
        if inference not in cache:
            from yolo_tf_amd import quant
            spec, params = seeded_params(inference)
            nodes = Q.plan(spec)
            images = np.random.RandomState(2).uniform(0, 255, (B, SIZE, SIZE, 3)).astype(np.float32)
            x = np.stack([R.per_image_standardization(i) for i in images]).astype(np.float32)
            acts = f32_activations(nodes, params, x)
            oracle = acts['conv'].astype(np.float64)
            classes = [sorted(c) for c in Q.scale_classes(nodes)]
            limits = [max(Q.absmax(acts[t])[0] for t in cls) for cls in classes]
            hists = [sum(C.abs_histogram(acts[t], limit)[0] for t in cls) for cls, limit in zip(classes, limits)]
            first = nodes[1]['out']
            rel = {}
            for method in ('absmax',) + METHODS:
                if method == 'absmax':
                    scales = Q.resolve_scales(nodes, {t: Q.absmax(acts[t])[0] for t in Q.int8_tensors(nodes)})
                else:
                    scales = quant.calibration_from_histograms(classes, limits, hists, method, 99.99)[0].scales
                out = Q.run(nodes, params, scales, first, Q.quantize(acts[first], Q.inv_scale(scales[first])))
                got = out['logits'].astype(np.float64)
                rel[method] = float(np.linalg.norm(got - oracle) / np.linalg.norm(oracle))
            cache[inference] = rel
        return cache[inference]
    return get


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('inference', ['tiny', 'darknet'])
def test_int8_logits_under_each_method_against_the_f32_oracle(nets, inference, method):
    """Twice the abs-max figure of the same run is the guard tests/test_quant_cpu.py uses against broken scales.  Measured (DESIGN.md section
    15): tiny absmax 0.0283, mse 0.0290, entropy 0.0318, percentile 0.0285; darknet absmax 0.0488, mse 0.0497, entropy 0.0689, percentile
    0.0494 -- on 8192 to 131072 values per class no method beats the abs-max; the device figures at 416 x 416 are in
    profiles/quant_calibration.md."""
    rel = nets(inference)
    print('int8 specification vs f32 oracle, %s %dx%d batch %d: relative L2 of the logits  absmax %.4f  %s %.4f' % (
        inference, SIZE, SIZE, B, rel['absmax'], method, rel[method]))
    assert rel[method] <= 2 * rel['absmax']
