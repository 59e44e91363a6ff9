"""The int8 specification (tests/quant_ref.py) on the CPU: scale classes, quantiser bounds, the accuracy of the ALGORITHM against the f32
oracle, the product's graph analysis against the specification's, and the argument checks of yolo2_conv2d_i8 (no GPU anywhere)."""
import os
import tempfile

import numpy as np
import pytest

import quant_ref as Q
from oracle import yolo2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES, ANCHORS, SIZE, B = 20, 5, 64, 2
# Relative L2 of the specification's logits against the f32 oracle's, calibrated on the same two images (measured by
# test_int8_logits_against_the_f32_oracle on the CPU, recorded in profiles/quant_int8.md).  The run is deterministic; the test allows twice
# the value for NumPy / BLAS differences between machines.
MEASURED_REL_L2 = {'tiny': 0.0283, 'darknet': 0.0488}


def seeded_params(inference, seed=1):
    """The oracle's seeded initial parameters with moving statistics and head biases off their defaults and fan-in scaled filters (what
    tests/test_network_gpu.py uses for inference: the tiny plugin's truncated_normal(0.1) overflows through nine inference-mode layers)."""
    spec = R.SPECS[inference](CLASSES, ANCHORS)
    params = R.init_params(spec, seed=0, tiny=inference == 'tiny')
    rng = np.random.RandomState(seed)
    for k in list(params):
        v = params[k]
        if k.endswith('moving_mean'):
            params[k] = (rng.randn(*v.shape) * 0.05).astype(np.float32)
        elif k.endswith('moving_variance'):
            params[k] = (rng.rand(*v.shape) + 0.5).astype(np.float32)
        elif k == 'conv/biases':
            params[k] = rng.randn(*v.shape).astype(np.float32)
        elif k.endswith('/weights'):
            kh, kw, cin, _ = v.shape
            params[k] = (rng.randn(*v.shape) * np.sqrt(2.0 / (kh * kw * cin))).astype(np.float32)
    return spec, params


def f32_activations(nodes, params, x):
    """Every tensor of the f32 network, by the oracle's own layer functions."""
    acts = {'input': x}
    for n in nodes:
        ins = [acts[t] for t in n['inputs']]
        if n['kind'] == 'conv':
            y = R.conv2d(ins[0], params[n['name'] + '/weights'])
            if n['bn']:
                p = n['name'] + '/BatchNorm/'
                y = R.leaky_relu(R.bn_apply(y, params[p + 'moving_mean'], params[p + 'moving_variance'], params[p + 'gamma'], params[p + 'beta']))
            else:
                y = y + params[n['name'] + '/biases']
            acts[n['out']] = y.astype(np.float32)
        elif n['kind'] == 'pool':
            acts[n['out']] = R.max_pool(ins[0], n['stride'])
        elif n['kind'] == 'reorg':
            acts[n['out']] = R.reorg(ins[0])
        elif n['kind'] == 'concat':
            acts[n['out']] = np.concatenate(ins, axis=3)
    return acts


@pytest.fixture(scope='module')
def nets():
    cache = {}

    def get(inference):
        if inference not in cache:
            spec, params = seeded_params(inference)
            nodes = Q.plan(spec)
            images = np.random.RandomState(2).uniform(0, 255, (B, SIZE, SIZE, 3)).astype(np.float32)
            x = np.stack([R.per_image_standardization(i) for i in images]).astype(np.float32)
            acts = f32_activations(nodes, params, x)
            oracle, _ = R.network_forward(spec, params, x, training=False)
            assert np.array_equal(acts['conv'], oracle)          # the walk above IS the oracle's network
            q = Q.int8_tensors(nodes)
            scales = Q.resolve_scales(nodes, {t: Q.absmax(acts[t])[0] for t in q})
            first = nodes[1]['out']
            out = Q.run(nodes, params, scales, first, Q.quantize(acts[first], Q.inv_scale(scales[first])))
            cache[inference] = dict(spec=spec, params=params, nodes=nodes, acts=acts, oracle=oracle, scales=scales, out=out, q=q)
        return cache[inference]
    return get


def test_scale_classes_are_the_stated_ones():
    tiny = Q.scale_classes(Q.plan(R.tiny_spec(CLASSES, ANCHORS)))
    dark = Q.scale_classes(Q.plan(R.darknet_spec(CLASSES, ANCHORS)))
    assert frozenset({'conv12', 'pool12', 'reorg', 'concat', 'conv19'}) in dark
    assert sorted(sorted(c) for c in dark if len(c) > 1) == [['concat', 'conv12', 'conv19', 'pool12', 'reorg'], ['conv1', 'pool1'], ['conv4', 'pool4'],
                                                             ['conv7', 'pool7']]
    assert sorted(sorted(c) for c in tiny if len(c) > 1) == [['conv%d' % i, 'pool%d' % i] for i in range(1, 6)]
    for classes in (tiny, dark):
        names = [t for c in classes for t in c]
        assert len(names) == len(set(names)) and 'conv0' not in names and 'conv' not in names and 'pool0' in names


def test_every_layer_but_the_image_layer_runs_in_int8():
    for spec in (R.tiny_spec, R.darknet_spec):
        convs = [n for n in Q.plan(spec(CLASSES, ANCHORS)) if n['kind'] == 'conv']
        assert [n['int8'] for n in convs] == [False] + [True] * (len(convs) - 1)
    # the long reduction the int32 headroom claim is about
    conv20 = [n for n in Q.plan(R.darknet_spec(CLASSES, ANCHORS)) if n['name'] == 'conv20'][0]
    assert conv20['cin'] == 3072 and 9 * 3072 * 127 * 127 < 2 ** 31


@pytest.mark.parametrize('inference', ['tiny', 'darknet'])
def test_product_graph_analysis_equals_the_specification(inference):
    """yolo_tf_amd.quant.QuantPlan over the traced graph: same int8 tensors, same classes (graph construction needs no GPU)."""
    from yolo_tf_amd import quant, utils
    from yolo_tf_amd.model import yolo2
    with tempfile.TemporaryDirectory() as basedir:
        cfg = utils.make_config([os.path.join(ROOT, 'config.ini'), os.path.join(ROOT, 'config', 'yolo2', '%s-%d.ini' % (inference, CLASSES))], basedir)
        cfg.set('cache', 'names', os.path.join(ROOT, cfg.get('cache', 'names')))
        cfg.set('yolo2', 'anchors', os.path.join(ROOT, cfg.get('yolo2', 'anchors')))
        utils.ensure_names(cfg)
        b = yolo2.Builder(None, cfg)
        b(None, training=False)
    plan = quant.QuantPlan(b.graph)
    nodes = Q.plan(R.SPECS[inference](CLASSES, ANCHORS))
    assert [n['kind'] for n in nodes] == [op['kind'] for op in b.graph.ops]
    name_of = {n['out']: op['out'].name for n, op in zip(nodes, b.graph.ops)}
    assert sorted(plan.names()) == sorted(name_of[t] for t in Q.int8_tensors(nodes))
    assert sorted(sorted(t.name for t in c) for c in plan.classes) == sorted(sorted(name_of[t] for t in c) for c in Q.scale_classes(nodes))


def test_yolo_v1_is_out_of_scope():
    from yolo_tf_amd import graph as G
    from yolo_tf_amd import quant
    g = G.Graph()
    net = G.placeholder(g, 'image', 8, 8)
    net = G.conv2d(net, 16, 3, scope='v1/conv0', batch_norm=False, activation=True)
    net = G.fully_connected(G.flatten(G.max_pool2d(net, 2, scope='v1/pool')), 10, scope='v1/fc', activation=False)
    with pytest.raises(NotImplementedError, match='v1'):
        quant.QuantPlan(g)


def quant_error_bound(x, am):
    half = np.asarray(am, np.float64) / 254
    return half + 2.0 ** -23 * (np.abs(np.asarray(x, np.float64)) + half)


def test_quantiser_error_bound():
    """|x - q * s| <= absmax / 254 plus one ulp, derived: s / 2 = (absmax / 254)(1 + d1) and fl(x * fl(1 / s)) = (x / s)(1 + d2)(1 + d3) with
    |d| <= 2^-24 each, so the error is at most absmax / 254 + 2^-23 (|x| + absmax / 254): the f32 machine epsilon (one ulp, relative) on the
    element and on the half step (quant_error_bound below)."""
    rng = np.random.RandomState(3)
    for scale in (1e-3, 1.0, 37.5):
        x = (rng.randn(20000) * scale).astype(np.float32)
        am, bad = Q.absmax(x)
        assert bad == 0 and am == np.abs(x).max()
        s = Q.scale_of(am)
        q = Q.quantize(x, Q.inv_scale(s))
        assert q.dtype == np.int8 and np.abs(q.astype(np.int32)).max() == 127 and q.min() >= -127
        err = np.abs(x.astype(np.float64) - q.astype(np.float64) * np.float64(s))
        assert (err <= quant_error_bound(x, am)).all()
    assert Q.scale_of(0) == 1 and Q.scale_of(np.inf) == 1 and Q.scale_of(np.nan) == 1
    special = Q.quantize(np.array([np.nan, np.inf, -np.inf, 0.5, -0.5, 1.5, 2.5], np.float32), np.float32(1))
    assert special.tolist() == [0, 127, -127, 0, 0, 2, 2]          # NaN -> 0, saturation, round half to even


@pytest.mark.parametrize('inference', ['tiny', 'darknet'])
def test_weight_round_trip(nets, inference):
    n = nets(inference)
    for node in n['nodes']:
        if node['kind'] != 'conv' or not node['int8']:
            continue
        wq, mult, bias, s_w = Q.layer_operands(node, n['params'], np.float32(1))
        name = node['name']
        if node['bn']:
            Wf, _ = Q.fold_bn(n['params'][name + '/weights'], n['params'][name + '/BatchNorm/gamma'], n['params'][name + '/BatchNorm/beta'],
                              n['params'][name + '/BatchNorm/moving_mean'], n['params'][name + '/BatchNorm/moving_variance'])
        else:
            Wf = n['params'][name + '/weights']
        assert wq.dtype == np.int8 and wq.min() >= -127 and (np.abs(wq.astype(np.int32)).reshape(-1, wq.shape[-1]).max(axis=0) == 127).all()
        err = np.abs(Wf.astype(np.float64) - wq.astype(np.float64) * s_w.astype(np.float64))
        assert (err <= quant_error_bound(Wf, np.abs(Wf).reshape(-1, Wf.shape[-1]).max(axis=0))).all(), name
        assert np.array_equal(mult, s_w)


@pytest.mark.parametrize('inference', ['tiny', 'darknet'])
def test_int8_logits_against_the_f32_oracle(nets, inference):
    n = nets(inference)
    got, ref = n['out']['logits'].astype(np.float64), n['oracle'].astype(np.float64)
    rel = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    print('int8 specification vs f32 oracle, %s %dx%d batch %d: relative L2 of the logits = %.4f' % (inference, SIZE, SIZE, B, rel))
    assert rel <= 2 * MEASURED_REL_L2[inference]
    # every int8 tensor uses its grid: the class scale puts the largest member at 127
    for cls in Q.scale_classes(n['nodes']):
        assert max(int(np.abs(n['out'][t].astype(np.int32)).max()) for t in cls if t in n['out']) >= 126, sorted(cls)


def test_calibration_file_round_trip(tmp_path):
    from yolo_tf_amd import quant
    c = quant.Calibration({'a/leaky_relu': np.float32(0.0123), 'b': np.float32(1)})
    path = str(tmp_path / 'calibration.npz')
    c.save(path)
    z = np.load(path)
    assert sorted(z.files) == ['names', 'scales'] and z['scales'].dtype == np.float32
    assert quant.Calibration.load(path) == c


def test_host_quantiser_of_the_product_equals_the_specification():
    from yolo_tf_amd import quant
    rng = np.random.RandomState(4)
    W = rng.randn(3, 3, 16, 24).astype(np.float32)
    W[..., 5] = 0                                                   # an all-zero filter: scale 1, all zeros
    gamma, beta = rng.rand(24).astype(np.float32) + 0.5, rng.randn(24).astype(np.float32)
    mean, var = rng.randn(24).astype(np.float32), rng.rand(24).astype(np.float32) + 0.1
    a, b = quant.fold_bn(W, gamma, beta, mean, var), Q.fold_bn(W, gamma, beta, mean, var)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    (qa, sa), (qb, sb) = quant.quantize_weights(a[0]), Q.quantize_weights(b[0])
    assert np.array_equal(qa, qb) and np.array_equal(sa, sb) and sa[5] == 1 and not qa[..., 5].any()


def test_conv2d_i8_argument_errors_raise_without_touching_the_gpu():
    from yolo_tf_amd import _lib
    ok = 1 << 20                                                    # a 16-byte aligned, never dereferenced address
    args = lambda P=ok, F=ok, Cp=32, ldp=32: (P, F, ok, ok, ok, 1, 4, 4, Cp, ldp, 16, 16, 3, 0.1, 1.0, 0, None)      # noqa: E731
    with pytest.raises(_lib.HipKernelError, match='argument check failed.*Cp % 16'):
        _lib.call('yolo2_conv2d_i8', *args(Cp=24, ldp=24))
    with pytest.raises(_lib.HipKernelError, match='argument check failed.*ldp'):
        _lib.call('yolo2_conv2d_i8', *args(Cp=32, ldp=40))
    with pytest.raises(_lib.HipKernelError, match='argument check failed.*15'):
        _lib.call('yolo2_conv2d_i8', *args(P=ok + 4))
    with pytest.raises(_lib.HipKernelError, match='argument check failed.*15'):
        _lib.call('yolo2_conv2d_i8', *args(F=ok + 8))
    with pytest.raises(_lib.HipKernelError, match='argument check failed'):
        _lib.call('yolo2_conv2d_i8', None, None, None, None, None, 1, 4, 4, 32, 32, 16, 16, 3, 0.1, 1.0, 0, None)
    with pytest.raises(_lib.HipKernelError, match='argument check failed.*out_kind'):
        _lib.call('yolo2_conv2d_i8', *(args()[:15] + (4, None)))
