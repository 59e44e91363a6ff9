"""int8 inference on the MI355X against the NumPy specification (tests/quant_ref.py): integer arithmetic and single-rounding f32 steps,
so everything here is compared bit for bit."""
import os
import tempfile

import numpy as np
import pytest
import torch

import quant_ref as Q
from oracle import yolo2_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def conv_int64(xq, wq):
    """The int64 NumPy convolution (SAME, stride 1): no floating point anywhere."""
    kh, kw, cin, cout = wq.shape
    b, h, w, _ = xq.shape
    xp = np.zeros((b, h + kh - 1, w + kw - 1, cin), np.int64)
    xp[:, kh // 2:kh // 2 + h, kw // 2:kw // 2 + w] = xq
    acc = np.zeros((b, h, w, cout), np.int64)
    for r in range(kh):
        for s in range(kw):
            acc += xp[:, r:r + h, s:s + w].reshape(-1, cin).dot(wq[r, s].astype(np.int64)).reshape(b, h, w, cout)
    return acc


def rand_i8(rng, shape):
    a = rng.randint(-128, 128, size=shape).astype(np.int8)
    flat = a.reshape(-1)
    flat[rng.randint(0, flat.size, size=max(3, flat.size // 50))] = 127
    flat[rng.randint(0, flat.size, size=max(3, flat.size // 50))] = -127
    flat[rng.randint(0, flat.size, size=max(3, flat.size // 50))] = -128
    return a


def filter_operand(wq):
    k, _, cin, cout = wq.shape
    return np.ascontiguousarray(wq.reshape(k * k, cin, cout).transpose(2, 0, 1)).reshape(-1)


OUT_DTYPE = {0: torch.int8, 1: torch.bfloat16, 2: torch.float32, 3: torch.int32}


def device_conv(xq, wq, kind, mult=None, bias=None, alpha=1.0, inv_s=1.0, ldp=None, poff=0, ldo=None, ooff=0, sentinel=None):
    """Runs yolo2_conv2d_i8; the input sits at channel offset poff of a [M][ldp] buffer whose other lanes hold 99, the output at channel
    offset ooff of a [M][ldo] buffer pre-filled with ``sentinel``.  -> the whole output buffer [M][ldo] as a NumPy array (bf16 as int16 bits)."""
    from yolo_tf_amd import ops
    b, h, w, cin = xq.shape
    nf, k = wq.shape[3], wq.shape[0]
    M = b * h * w
    ldp = ldp or cin
    ldo = ldo or nf
    pbuf = np.full((M, ldp), 99, np.int8)
    pbuf[:, poff:poff + cin] = xq.reshape(M, cin)
    P = torch.from_numpy(pbuf.reshape(-1)).cuda()
    F = torch.from_numpy(filter_operand(wq)).cuda()
    O = torch.zeros(M * ldo, dtype=OUT_DTYPE[kind], device='cuda')
    if sentinel is not None:
        O.fill_(sentinel)
    mt = None if mult is None else torch.from_numpy(np.asarray(mult, np.float32)).cuda()
    bt = None if bias is None else torch.from_numpy(np.asarray(bias, np.float32)).cuda()
    ops.conv2d_i8(P[poff:], F, mt, bt, O[ooff:], b, h, w, cin, ldp, nf, ldo, k, alpha, inv_s, kind)
    torch.cuda.synchronize()
    if kind == 1:
        O = O.view(torch.int16)
    return O.cpu().numpy().reshape(M, ldo)


# ---- convolution, raw accumulators --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('nf', [16, 40, 125])
@pytest.mark.parametrize('cin', [16, 32, 80])
def test_conv_i8_accumulators_equal_int64_numpy(cin, nf, k):
    """Also what establishes the operand lane map of v_mfma_i32_32x32x32_i8: exact integer data, an asymmetric (random) filter, channel
    counts that are not a multiple of the 64-byte K step, filter counts that are not a multiple of the tile."""
    rng = np.random.RandomState(cin * 1000 + nf * 10 + k)
    xq, wq = rand_i8(rng, (2, 5, 7, cin)), rand_i8(rng, (k, k, cin, nf))
    got = device_conv(xq, wq, 3)
    assert np.array_equal(got.reshape(2, 5, 7, nf).astype(np.int64), conv_int64(xq, wq))


def test_conv_i8_strides_channel_offsets_and_sentinels():
    rng = np.random.RandomState(7)
    xq, wq = rand_i8(rng, (2, 5, 7, 32)), rand_i8(rng, (3, 3, 32, 40))
    got = device_conv(xq, wq, 3, ldp=64, poff=16, ldo=64, ooff=8, sentinel=-77)
    assert np.array_equal(got[:, 8:48].reshape(2, 5, 7, 40).astype(np.int64), conv_int64(xq, wq))
    assert (got[:, :8] == -77).all() and (got[:, 48:] == -77).all()


def test_conv_i8_more_than_one_pixel_tile_with_a_tail():
    rng = np.random.RandomState(8)
    xq, wq = rand_i8(rng, (3, 13, 13, 32)), rand_i8(rng, (3, 3, 32, 40))        # M = 507 = 3 tiles of 128 + 123
    got = device_conv(xq, wq, 3, ldo=48, sentinel=-77)
    assert np.array_equal(got[:, :40].reshape(3, 13, 13, 40).astype(np.int64), conv_int64(xq, wq))
    assert (got[:, 40:] == -77).all()


def test_conv_i8_longest_reduction_stays_inside_int32():
    """conv20 of darknet: 9 * 3072 terms of 127 * 127 = 445 934 592 < 2^31."""
    rng = np.random.RandomState(9)
    xq = np.where(rng.rand(1, 2, 2, 3072) < 0.5, -127, 127).astype(np.int8)
    wq = np.where(rng.rand(3, 3, 3072, 16) < 0.5, -127, 127).astype(np.int8)
    xq[0, 0, 0] = 127
    wq[:, :, :, 0] = 127                 # filter 0 against an all-127 pixel: the centre-of-mass worst case of the 4 taps inside a 2x2 image
    got = device_conv(xq, wq, 3).reshape(1, 2, 2, 16).astype(np.int64)
    assert np.array_equal(got, conv_int64(xq, wq))
    # the full 9-tap worst case needs an interior pixel: 3x3 image, everything 127
    xq = np.full((1, 3, 3, 3072), 127, np.int8)
    wq = np.full((3, 3, 3072, 16), 127, np.int8)
    wq[:, :, :, 1] = -127
    got = device_conv(xq, wq, 3).reshape(1, 3, 3, 16).astype(np.int64)
    assert got[0, 1, 1, 0] == 9 * 3072 * 127 * 127 and got[0, 1, 1, 1] == -9 * 3072 * 127 * 127
    assert np.array_equal(got, conv_int64(xq, wq))


# ---- convolution with the epilogue ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('leaky', [True, False])
@pytest.mark.parametrize('kind', [0, 1], ids=['int8', 'bf16'])
def test_conv_i8_epilogue_bit_equal(kind, leaky):
    rng = np.random.RandomState(10 + kind * 2 + leaky)
    xq, wq = rand_i8(rng, (2, 5, 7, 32)), rand_i8(rng, (3, 3, 32, 40))
    mult = (rng.rand(40) * 2e-4 + 1e-5).astype(np.float32)
    bias = rng.randn(40).astype(np.float32)
    inv_s = np.float32(1) / np.float32(0.031)              # some outputs saturate at +-127
    y = Q.conv_epilogue(Q.conv_acc(xq, wq), mult, bias, leaky=leaky)
    got = device_conv(xq, wq, kind, mult, bias, alpha=float(Q.ALPHA) if leaky else 1.0, inv_s=inv_s)
    if kind == 0:
        want = Q.quantize(y, inv_s).reshape(-1, 40)
        assert (np.abs(want) == 127).any() and (np.abs(want) < 127).any()
        assert np.array_equal(got, want)
    else:
        assert np.array_equal(got.view(np.uint16), Q.bf16_bits(y).reshape(-1, 40))


def test_conv_i8_f32_output():
    rng = np.random.RandomState(20)
    xq, wq = rand_i8(rng, (2, 5, 7, 16)), rand_i8(rng, (1, 1, 16, 16))
    mult, bias = (rng.rand(16) * 1e-3).astype(np.float32), rng.randn(16).astype(np.float32)
    got = device_conv(xq, wq, 2, mult, bias, alpha=float(Q.ALPHA))
    assert np.array_equal(got, Q.conv_epilogue(Q.conv_acc(xq, wq), mult, bias).reshape(-1, 16))


# ---- elementwise kernels --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_quantize_bit_equal_on_odd_sizes_and_strides(dtype):
    from yolo_tf_amd import ops
    rng = np.random.RandomState(30)
    rows, c, ldx, ldq = 37, 13, 19, 24
    x = (rng.randn(rows, ldx) * 3).astype(np.float32)
    x[0, 0], x[1, 1], x[2, 2], x[3, 3], x[4, 4] = np.nan, np.inf, -np.inf, 1e30, -1e30
    X = torch.from_numpy(x).cuda().to(dtype)
    xs = X.float().cpu().numpy()                           # what the kernel reads (bf16: the rounded values)
    Qd = torch.full((rows * ldq,), -77, dtype=torch.int8, device='cuda')
    inv_s = Q.inv_scale(Q.scale_of(np.float32(7.3)))
    ops.quantize(X.reshape(-1), ldx, Qd, ldq, rows, c, inv_s)
    got = Qd.cpu().numpy().reshape(rows, ldq)
    assert np.array_equal(got[:, :c], Q.quantize(xs[:, :c], inv_s))
    assert got[0, 0] == 0 and got[1, 1] == 127 and got[2, 2] == -127
    assert (got[:, c:] == -77).all()


@pytest.mark.parametrize('h,w,c,stride', [(5, 7, 16, 2), (5, 7, 5, 2), (13, 13, 32, 1), (13, 13, 3, 1), (4, 6, 16, 2)])
def test_maxpool_i8(h, w, c, stride):
    from yolo_tf_amd import ops
    rng = np.random.RandomState(40)
    x = rand_i8(rng, (2, h, w, c))
    want = Q.max_pool(x, stride)
    oh, ow = want.shape[1:3]
    out = torch.full((2 * oh * ow * c,), -77, dtype=torch.int8, device='cuda')
    ops.maxpool_i8(torch.from_numpy(x.reshape(-1)).cuda(), c, out, c, 2, h, w, c, stride)
    assert np.array_equal(out.cpu().numpy().reshape(want.shape), want)


def test_maxpool_i8_matches_the_float_pool_of_the_oracle():
    """The byte pool is the oracle's SAME pool: quantising commutes with it."""
    rng = np.random.RandomState(41)
    x = rng.randn(2, 13, 13, 8).astype(np.float32)
    inv_s = Q.inv_scale(Q.scale_of(Q.absmax(x)[0]))
    for stride in (1, 2):
        xe = x if stride == 1 else x[:, :12, :12]
        assert np.array_equal(Q.max_pool(Q.quantize(xe, inv_s), stride), Q.quantize(R.max_pool(xe, stride), inv_s))


def test_reorg_i8_with_output_stride():
    from yolo_tf_amd import ops
    rng = np.random.RandomState(50)
    x = rand_i8(rng, (2, 4, 6, 16))
    out = torch.full((2 * 2 * 3 * 80,), -77, dtype=torch.int8, device='cuda')
    ops.reorg_i8(torch.from_numpy(x.reshape(-1)).cuda(), out, 2, 4, 6, 16, 80)
    got = out.cpu().numpy().reshape(2, 2, 3, 80)
    assert np.array_equal(got[..., :64], Q.reorg(x)) and np.array_equal(Q.reorg(x), R.reorg(x))
    assert (got[..., 64:] == -77).all()


def test_absmax_three_tensors_two_batches():
    from yolo_tf_amd import ops
    rng = np.random.RandomState(60)
    a = torch.zeros(31 * 17, dtype=torch.float32, device='cuda')             # dense f32
    b = torch.zeros(29 * 24, dtype=torch.bfloat16, device='cuda')            # bf16, 13 of every 24
    c = torch.zeros(500 * 40, dtype=torch.float32, device='cuda')            # f32, 33 of every 40
    jobs = ops.AbsmaxJobs([(a, 31, 17, 17, 0), (b, 29, 13, 24, 1), (c, 500, 33, 40, 2)], 3)
    want, bad = np.zeros(3, np.float32), np.zeros(3, np.int64)
    for batch in range(2):
        hosts = []
        for t, (rows, cc, ld) in zip((a, b, c), ((31, 17, 17), (29, 13, 24), (500, 33, 40))):
            x = (rng.randn(rows, ld) * (3.0 if batch == 0 else 1.0 + t.numel() % 7)).astype(np.float32)
            x[:, cc:] = 1e6                                   # lanes outside the job must not be read
            x[1, 0], x[2, 1] = np.nan, (np.inf if batch else -np.inf)
            t.copy_(torch.from_numpy(x.reshape(-1)).cuda().to(t.dtype))
            hosts.append(t.float().cpu().numpy().reshape(rows, ld)[:, :cc])
        jobs.launch()
        for i, x in enumerate(hosts):
            m, n = Q.absmax(x)
            want[i] = max(want[i], m)
            bad[i] += n
        got, got_bad = jobs.result()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(got_bad, bad)
    assert (bad == 4).all()


# ---- whole network --------------------------------------------------------------------------------------------------------------------------

def make_builder(inference, names, size, basedir):
    from yolo_tf_amd import utils
    from yolo_tf_amd.model import yolo2
    cfg = utils.make_config([os.path.join(ROOT, 'config.ini'), os.path.join(ROOT, 'config', 'yolo2', '%s-%d.ini' % (inference, names))], basedir)
    cfg.set('cache', 'names', os.path.join(ROOT, cfg.get('cache', 'names')))
    cfg.set('yolo2', 'anchors', os.path.join(ROOT, cfg.get('yolo2', 'anchors')))
    cfg.set('yolo2', 'width', str(size))
    cfg.set('yolo2', 'height', str(size))
    utils.ensure_names(cfg)
    b = yolo2.Builder(None, cfg)
    b(None, training=False)
    return b


def seeded_params(variables, seed=1):
    """The engine's seeded initial variables with the moving statistics and the head's biases moved off their defaults and fan-in scaled
    filters (the tiny plugin's truncated_normal(0.1) overflows through nine inference-mode layers: tests/test_network_gpu.py)."""
    rng = np.random.RandomState(seed)
    out = {}
    for k, v in variables.items():
        if k.endswith('moving_mean'):
            v = (rng.randn(*v.shape) * 0.05).astype(np.float32)
        elif k.endswith('moving_variance'):
            v = (rng.rand(*v.shape) + 0.5).astype(np.float32)
        elif k.endswith('conv/biases'):
            v = rng.randn(*v.shape).astype(np.float32)
        elif k.endswith('/weights'):
            kh, kw, cin, _ = v.shape
            v = (rng.randn(*v.shape) * np.sqrt(2.0 / (kh * kw * cin))).astype(np.float32)
        out[k] = v
    return out


@pytest.fixture(scope='module')
def networks():
    """Per network: the bf16 session, the device calibration, the int8 session's tensors and the specification's, computed once."""
    cache = {}

    def get(inference):
        if inference in cache:
            return cache[inference]
        from yolo_tf_amd import quant
        from yolo_tf_amd.session import DetectSession
        B, size, classes = 2, 64, 20
        with tempfile.TemporaryDirectory() as basedir:
            b = make_builder(inference, classes, size, basedir)
            b8 = make_builder(inference, classes, size, basedir)
        sess = DetectSession(b, B, dtype='bf16', seed=5)
        values = seeded_params(sess.engine.get_variables())
        sess.engine.set_variables(values)
        images = torch.from_numpy(np.random.RandomState(2).uniform(0, 255, (B, size, size, 3)).astype(np.float32)).cuda()
        cal = quant.Calibrator(sess)
        cal.observe(images)
        torch.cuda.synchronize()
        e = cal.engine
        host = {}
        for t in cal.plan.tensors:
            buf, ld = e.act[t]
            rows = B * t.h * t.w
            flat = buf[:(rows - 1) * ld + t.c].float().cpu().numpy()
            host[t.name] = np.concatenate([flat, np.zeros(rows * ld - flat.size, np.float32)]).reshape(rows, ld)[:, :t.c]
        calibration = cal.finish()
        sess8 = DetectSession(b8, B, dtype='int8', seed=5, calibration=calibration)
        sess8.engine.set_variables(values)
        conf, mn, mx, order = [t.clone() for t in sess8.detect(images, threshold=0.02, threshold_iou=0.4)]
        torch.cuda.synchronize()
        e8 = sess8.engine
        dev = {}
        for t in e8.plan.tensors:
            buf, ld = e8.act[t]
            rows = B * t.h * t.w
            flat = buf[:(rows - 1) * ld + t.c].cpu().numpy()
            dev[t.name] = np.concatenate([flat, np.zeros(rows * ld - flat.size, np.int8)]).reshape(rows, ld)[:, :t.c].reshape(B, t.h, t.w, t.c)
        out = e8.output()
        buf, ld = e8.act[out]
        logits_bits = buf[:B * out.h * out.w * ld].view(torch.int16).cpu().numpy().view(np.uint16).reshape(B, out.h, out.w, ld)[..., :out.c]
        # the specification on the same variables, from the device's first int8 tensor on
        scope = 'yolo2_' + inference
        nodes = Q.plan(R.SPECS[inference](classes, 5))
        graph_ops = b8.graph.ops
        assert [n['kind'] for n in nodes] == [op['kind'] for op in graph_ops]
        name_of = {n['out']: op['out'].name for n, op in zip(nodes, graph_ops)}
        params = {k[len(scope) + 1:]: v for k, v in values.items()}
        scales = {n: calibration.scales[name_of[n]] for n in Q.int8_tensors(nodes)}
        first = nodes[1]['out']
        spec = Q.run(nodes, params, scales, first, dev[name_of[first]])
        cache[inference] = dict(sess=sess, sess8=sess8, cal=cal, calibration=calibration, host=host, dev=dev, logits_bits=logits_bits, nodes=nodes,
                                name_of=name_of, spec=spec, detect=(conf, mn, mx, order), B=B, classes=classes, builder=b8)
        return cache[inference]
    return get


@pytest.mark.parametrize('inference', ['tiny', 'darknet'])
def test_device_scales_equal_numpy_absmax_of_the_bf16_activations(networks, inference):
    n = networks(inference)
    amax, bad = n['cal'].absmax()
    assert bad == 0
    for name, x in n['host'].items():
        assert np.float32(amax[name]).view(np.uint32) == Q.absmax(x)[0].view(np.uint32), name
    want = Q.resolve_scales(n['nodes'], {k: amax[n['name_of'][k]] for k in Q.int8_tensors(n['nodes'])})
    assert {n['name_of'][k]: v for k, v in want.items()} == n['calibration'].scales
    got_classes = sorted(sorted(t.name for t in cls) for cls in n['cal'].plan.classes)
    assert got_classes == sorted(sorted(n['name_of'][k] for k in cls) for cls in Q.scale_classes(n['nodes']))


@pytest.mark.parametrize('inference', ['tiny', 'darknet'])
def test_every_int8_activation_and_the_logits_equal_the_specification(networks, inference):
    n = networks(inference)
    checked = 0
    for k, want in n['spec'].items():
        if k in ('logits', 'logits_bits'):
            continue
        assert np.array_equal(n['dev'][n['name_of'][k]], want), k
        checked += 1
    assert checked == len(n['dev'])
    assert np.array_equal(n['logits_bits'], n['spec']['logits_bits'])
    used = [np.abs(v).max() for k, v in n['spec'].items() if k not in ('logits', 'logits_bits')]
    assert max(used) == 127 and min(used) > 16          # the scales put the data on the int8 grid, no tensor collapsed to a few levels


@pytest.mark.parametrize('inference', ['tiny', 'darknet'])
def test_detect_session_int8_keeps_what_the_specification_keeps(networks, inference):
    """decode + NMS of the specification's logits (uploaded as the bf16 values they are) through the same kernels: same scores, same order."""
    from yolo_tf_amd import ops
    n = networks(inference)
    s8, B, C = n['sess8'], n['B'], n['classes']
    conf, mn, mx, order = n['detect']
    m = s8.model
    bits = n['spec']['logits_bits']
    ld = (bits.shape[-1] + 7) // 8 * 8
    padded = np.zeros(bits.shape[:-1] + (ld,), np.uint16)
    padded[..., :bits.shape[-1]] = bits
    logits = torch.from_numpy(padded.view(np.int16).reshape(-1)).cuda().view(torch.bfloat16)
    conf2, mn2, mx2 = torch.zeros_like(conf), torch.zeros_like(mn), torch.zeros_like(mx)
    order2, flag = torch.zeros_like(order), torch.zeros(1, dtype=torch.int32, device='cuda')
    ops.head_decode(logits, ld, s8.anchors, conf2, mn2, mx2, flag, B, m.cell_height, m.cell_width, s8.A, C)
    ws = torch.zeros(ops.workspace_bytes('nms', B, s8.N, C) // 4, dtype=torch.int32, device='cuda')
    ops.nms(conf2, mn2, mx2, order2, ws, B, s8.N, C, 0.02, 0.4)
    assert int(flag.item()) == 0
    assert torch.equal(conf, conf2) and torch.equal(order, order2) and torch.equal(mn, mn2) and torch.equal(mx, mx2)
    assert bool((conf > 0.02).any()), 'the comparison is vacuous without a kept box'


def test_int8_session_needs_a_calibration_and_a_yolo2_graph():
    from yolo_tf_amd.session import DetectSession
    with tempfile.TemporaryDirectory() as basedir:
        b = make_builder('tiny', 20, 64, basedir)
    with pytest.raises(ValueError, match='calibration'):
        DetectSession(b, 1, dtype='int8')
