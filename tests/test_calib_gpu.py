"""yolo2_calib_histogram and the calibration methods on the MI355X against the NumPy specification (tests/calib_ref.py): the kernel is one
f32 multiply and integer arithmetic, so every record is compared bit for bit, with no tolerance."""
import logging
import tempfile

import numpy as np
import pytest
import torch

import calib_ref as C
import quant_ref as Q

pytestmark = pytest.mark.gpu
BINS, WORDS = C.BINS, C.BINS + 2
DTYPES = [torch.float32, torch.bfloat16]
IDS = ['f32', 'bf16']


def upload(x, dtype, offset=0):
    """-> (device tensor that holds x behind ``offset`` leading elements, the f32 values the kernel reads)"""
    t = torch.zeros(offset + x.size, dtype=dtype, device='cuda')
    t[offset:] = torch.from_numpy(np.ascontiguousarray(x, np.float32).reshape(-1)).to(dtype).cuda()      # converted on the host: denormals stay
    return t, t[offset:].cpu().float().numpy().reshape(x.shape)


def device_histogram(jobs, nslots):
    """jobs: [(tensor, rows, c, ld, slot, limit)] -> the whole records after one launch, uint64 [nslots, WORDS]"""
    from yolo_tf_amd import ops
    j = ops.CalibHistogramJobs(jobs, nslots)
    j.launch()
    torch.cuda.synchronize()
    return j.out.cpu().numpy().view(np.uint64)


def record(x, limit):
    h, nonfinite, clamped = C.abs_histogram(x, limit)
    return np.concatenate([h, [nonfinite, clamped]]).astype(np.uint64)


def data(rng, rows, ld, scale=1.0):
    """Leaky-normal values (most of them in the lowest bins) with a few outliers."""
    x = rng.standard_normal((rows, ld)).astype(np.float32) * np.float32(scale)
    x = np.where(x > 0, x, x * np.float32(0.1)).astype(np.float32)
    x.reshape(-1)[::97] *= np.float32(3)
    return x


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('rows,c,ld', [(1, 1, 1), (1, 5, 5), (1, 64, 64), (37, 1, 1), (37, 3, 3), (1031, 17, 17), (1031, 17, 24), (37, 3, 8), (129, 64, 64),
                                       (129, 64, 80), (5000, 64, 64), (33, 1, 2)])
def test_histogram_equals_the_specification(dtype, rows, c, ld):
    """rows * c below one vector, below and above one chunk of a workgroup (8192 vectors), dense and strided, vector and scalar paths."""
    rng = np.random.RandomState(rows * 100 + c + ld)
    x = data(rng, rows, ld)
    x[:, c:] = 1e6                                                   # lanes outside the job must not be read
    t, x = upload(x, dtype)
    limit = Q.absmax(x[:, :c])[0]
    got = device_histogram([(t, rows, c, ld, 0, limit)], 1)
    want = record(x[:, :c], limit)
    assert np.array_equal(got[0], want)
    assert int(got[0, :BINS].sum()) == rows * c and got[0, BINS] == 0 and got[0, BINS + 1] == 0 and got[0, BINS - 1] >= 1


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('rows,c,ld', [(1031, 17, 17), (1031, 17, 24), (600, 64, 64), (600, 64, 72)])
def test_misaligned_base(dtype, rows, c, ld):
    """The base one element behind a 16-byte boundary: the scalar path, dense and strided."""
    rng = np.random.RandomState(7)
    t, x = upload(data(rng, rows, ld), dtype, offset=1)
    assert t.data_ptr() % 16 == 0 and t[1:].data_ptr() % 16 != 0
    limit = np.float32(2.5)
    got = device_histogram([(t[1:], rows, c, ld, 0, limit)], 1)
    assert np.array_equal(got[0], record(x[:, :c], limit)) and got[0, BINS + 1] > 0


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_more_chunks_than_workgroups(dtype):
    """A job of more than 256 chunks: a workgroup counts, flushes and zeroes its LDS copies more than once."""
    n = (256 * 8192 * (4 if dtype == torch.float32 else 8)) + 8192 * 9 + 5
    rng = np.random.RandomState(11)
    x = rng.standard_normal(n).astype(np.float32)
    t, x = upload(x, dtype)
    limit = Q.absmax(x)[0]
    got = device_histogram([(t, 1, n, n, 0, limit)], 1)
    assert np.array_equal(got[0], record(x, limit)) and int(got[0, :BINS].sum()) == n


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_bin_edges_limit_and_values_above_it(dtype):
    """Values exactly on the edges k * w (limit a power of two: the edges are exact in bf16 too), the limit itself, values above it."""
    limit = np.float32(8.0)
    w = np.float32(8.0 / BINS)
    k = np.arange(0, BINS + 1, dtype=np.float32)
    if dtype == torch.bfloat16:
        k = k[(k.view(np.uint32) & 0xffff) == 0]                     # the multiples a bf16 holds exactly
    edges = k * w
    below = np.nextafter(edges[1:], np.float32(0)) if dtype == torch.float32 else edges[1:] * np.float32(1 - 2.0 ** -8)
    x = np.concatenate([edges, -edges, below, [8.0, -8.0, 8.5, -1e30, 3e38, np.nextafter(np.float32(8), np.float32(9))]]).astype(np.float32)
    t, xs = upload(x, dtype)
    got = device_histogram([(t, 1, x.size, x.size, 0, limit)], 1)
    want = record(xs, limit)
    assert np.array_equal(got[0], want)
    if dtype == torch.float32:
        # an edge value opens its bin: bins 1 .. 2046 hold +k w, -k w and the value just below (k + 1) w; the last bin also the limit and beyond
        assert (got[0, 1:BINS - 1] == 3).all() and got[0, 0] == 3 and got[0, BINS - 1] == 3 + 2 + 2 + 4 and got[0, BINS + 1] == 4
    else:
        assert got[0, BINS + 1] == 3 and got[0, BINS - 1] >= 2 + 2 + 3


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_zeros_denormals_and_non_finite_values(dtype):
    # 8.816e-39 = 0.75 * 2^-126, a denormal in both formats: under the small limit it lands in bin 1, flushed to zero it would land in bin 0
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-39, 2.0 ** -126, -0.75 * 2.0 ** -126, np.nan, -np.nan, np.inf, -np.inf], np.float32)
    x = np.concatenate([special, np.linspace(-1, 1, 300, dtype=np.float32), special])
    t, xs = upload(x, dtype)
    # a tiny limit too: inv_width = 2048 / 2^-116 = 2^127 is the largest finite power of two
    for limit in (np.float32(1.0), np.float32(2.0 ** -116)):
        got = device_histogram([(t, 1, x.size, x.size, 0, limit)], 1)
        assert np.array_equal(got[0], record(xs, limit)), limit
        assert got[0, BINS] == 8 and int(got[0, :BINS].sum()) == x.size - 8
    assert got[0, 1] == 2 and got[0, 2] == 2                        # +-0.75 * 2^-126 -> t = 1.5; +-2^-126 -> t = 2
    assert device_histogram([(t, 1, x.size, x.size, 0, np.float32(1.0))], 1)[0, 0] == 16


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_all_values_equal_is_counted_exactly(dtype):
    """2**20 equal values: every lane of every wave adds to one LDS word."""
    n = 2 ** 20
    t = torch.full((n,), 0.75, dtype=dtype, device='cuda')
    got = device_histogram([(t, 1, n, n, 0, np.float32(1.0))], 1)
    want = np.zeros(WORDS, np.uint64)
    want[int(0.75 * BINS)] = n
    assert np.array_equal(got[0], want)
    # the same through the strided path, where a wave's lanes do not all hold an element at the end
    got = device_histogram([(t, n // 24, 17, 24, 0, np.float32(1.0))], 1)
    want[int(0.75 * BINS)] = n // 24 * 17
    assert np.array_equal(got[0], want)


def test_jobs_share_a_slot_and_slots_are_separate():
    rng = np.random.RandomState(21)
    a, xa = upload(data(rng, 301, 17), torch.float32)
    b, xb = upload(data(rng, 77, 24, 2.0), torch.bfloat16)
    c, xc = upload(data(rng, 500, 40, 0.5), torch.float32)
    la, lc = max(Q.absmax(xa)[0], Q.absmax(xb[:, :13])[0]), np.float32(1.0)
    got = device_histogram([(a, 301, 17, 17, 2, la), (c, 500, 33, 40, 0, lc), (b, 77, 13, 24, 2, la)], 3)
    assert np.array_equal(got[2], record(xa, la) + record(xb[:, :13], la))
    assert np.array_equal(got[0], record(xc[:, :33], lc)) and got[0, BINS + 1] > 0
    assert not got[1].any()


def test_successive_calls_accumulate_and_carry_into_the_high_word():
    from yolo_tf_amd import ops
    rng = np.random.RandomState(22)
    t = torch.zeros(1031 * 17, dtype=torch.bfloat16, device='cuda')
    jobs = ops.CalibHistogramJobs([(t, 1031, 17, 17, 0, np.float32(4.0))], 1)
    seed = np.zeros((1, WORDS), np.uint64)
    seed[0, 0] = 2 ** 32 - 1                                        # the lowest bin, which every batch below adds to
    seed[0, BINS + 1] = 2 ** 32 - 1
    jobs.out.copy_(torch.from_numpy(seed.view(np.int64)).cuda())
    want = seed[0].copy()
    for batch in range(2):
        x = data(rng, 1031, 17, 1.0 + batch)
        x[batch, 3] = np.nan
        t.copy_(torch.from_numpy(x.reshape(-1)).cuda().to(torch.bfloat16))
        jobs.launch()
        want = want + record(t.float().cpu().numpy(), np.float32(4.0))
        torch.cuda.synchronize()
        assert np.array_equal(jobs.out.cpu().numpy().view(np.uint64)[0], want)
    assert want[0] > 2 ** 32 and want[BINS + 1] > 2 ** 32 and want[BINS] == 2
    h, nonfinite, clamped = jobs.result()
    assert h.dtype == np.int64 and h.shape == (1, BINS) and nonfinite[0] == 2 and clamped[0] == int(want[BINS + 1]) and h[0, 0] == int(want[0])


def test_two_runs_are_identical():
    rng = np.random.RandomState(23)
    t, x = upload(data(rng, 4099, 64), torch.bfloat16)
    u, _ = upload(data(rng, 1031, 24), torch.float32)
    jobs = [(t, 4099, 64, 64, 0, np.float32(3.0)), (u, 1031, 17, 24, 0, np.float32(3.0)), (u, 1031, 17, 24, 1, np.float32(0.5))]
    first, second = device_histogram(jobs, 2), device_histogram(jobs, 2)
    assert np.array_equal(first, second) and first.any()


def test_argument_errors_and_host_asserts():
    from yolo_tf_amd import _lib, ops
    t = torch.zeros(64, dtype=torch.float32, device='cuda')
    j = ops.CalibHistogramJobs([(t, 4, 16, 16, 0, np.float32(1))], 1)
    for args in ((None, 1, j.out.data_ptr(), None), (j.table.data_ptr(), 1, None, None), (j.table.data_ptr(), 0, j.out.data_ptr(), None),
                 (j.table.data_ptr(), 65536, j.out.data_ptr(), None)):
        with pytest.raises(_lib.HipKernelError, match='argument check failed'):
            _lib.call('yolo2_calib_histogram', *args)
    torch.cuda.synchronize()
    assert not j.out.any()
    for bad in ((t, 4, 16, 16, 0, 0.0), (t, 4, 16, 16, 0, np.inf), (t, 4, 16, 16, 0, np.nan), (t, 4, 16, 16, 0, -1.0), (t, 4, 16, 16, 0, 1e-38),
                (t, 5, 16, 16, 0, 1.0), (t, 4, 16, 8, 0, 1.0), (t, 4, 16, 16, 1, 1.0)):
        with pytest.raises(AssertionError):
            ops.CalibHistogramJobs([bad], 1)
    with pytest.raises(AssertionError, match='disagree'):
        ops.CalibHistogramJobs([(t, 2, 16, 16, 0, 1.0), (t, 2, 16, 16, 0, 2.0)], 1)


# ---- the calibrator ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def tiny():
    """Seeded `tiny` at 64x64, batch 2: the session, one batch of images, and the calibrator's two passes observed once for 'mse'."""
    from test_quant_gpu import make_builder, seeded_params
    from yolo_tf_amd import quant
    from yolo_tf_amd.session import DetectSession
    B, size = 2, 64
    with tempfile.TemporaryDirectory() as basedir:
        b = make_builder('tiny', 20, size, basedir)
        b8 = make_builder('tiny', 20, size, basedir)
    sess = DetectSession(b, B, dtype='bf16', seed=5)
    values = seeded_params(sess.engine.get_variables())
    sess.engine.set_variables(values)
    images = torch.from_numpy(np.random.RandomState(2).uniform(0, 255, (B, size, size, 3)).astype(np.float32)).cuda()
    cal = quant.Calibrator(sess, method='mse')
    cal.observe(images)
    cal.observe_histogram(images)
    return dict(sess=sess, builder8=b8, values=values, images=images, cal=cal, B=B)


def activations(cal):
    """{tensor name: f32 [rows, c]}: what the calibrator's engine holds after its last forward pass."""
    torch.cuda.synchronize()
    e, host = cal.engine, {}
    for t in cal.plan.tensors:
        buf, ld = e.act[t]
        rows = e.B * t.h * t.w
        flat = buf[:(rows - 1) * ld + t.c].float().cpu().numpy()
        host[t.name] = np.concatenate([flat, np.zeros(rows * ld - flat.size, np.float32)]).reshape(rows, ld)[:, :t.c]
    return host


def host_calibration(cal, method, percentile=99.99):
    """The Calibration the host computes from the calibrator engine's own activations: specification histograms, the product's rule."""
    from yolo_tf_amd import quant
    host = activations(cal)
    classes = [[t.name for t in cls] for cls in cal.plan.classes]
    limits = [max(Q.absmax(host[name])[0] for name in cls) for cls in classes]
    hists = [sum(C.abs_histogram(host[name], limit)[0] for name in cls) for cls, limit in zip(classes, limits)]
    return quant.calibration_from_histograms(classes, limits, hists, method, percentile)[0], limits, hists


def test_calibrator_records_equal_the_specification_histograms(tiny):
    cal = tiny['cal']
    want, limits, hists = host_calibration(cal, 'mse')
    assert [np.float32(v).view(np.uint32) for v in cal.limits] == [np.float32(v).view(np.uint32) for v in limits]
    h, clamped = cal.histograms()
    assert np.array_equal(h, np.stack(hists)) and not clamped.any()
    for k, cls in enumerate(cal.plan.classes):
        assert int(h[k].sum()) == sum(tiny['B'] * t.h * t.w * t.c for t in cls)
    got = cal.finish()
    assert got == want and got.method == 'mse' and set(got.thresholds) == set(cal.plan.names())
    assert any(got.thresholds[n] < got.amax[n] for n in got.scales), 'mse clipped nothing: the comparison says little'
    assert len(cal.report) == len(cal.plan.classes)
    with pytest.raises(RuntimeError, match='frozen'):
        cal.observe(tiny['images'])


@pytest.mark.parametrize('method', ['percentile', 'entropy'])
def test_calibrate_with_each_method_equals_the_host(tiny, method):
    from yolo_tf_amd import quant
    cal = quant.Calibrator(tiny['sess'], method=method, percentile=99.9)
    cal.observe(tiny['images'])
    cal.observe_histogram(tiny['images'])
    want, _, _ = host_calibration(cal, method, 99.9)
    got = cal.finish()
    assert got == want and got.method == method
    # calibrate() does the same two passes; a one-shot iterator is gone over twice
    assert quant.calibrate(tiny['sess'], iter([tiny['images']]), method=method, percentile=99.9) == got


def test_absmax_method_allocates_no_histogram_and_other_methods_need_the_second_pass(tiny):
    from yolo_tf_amd import quant
    cal = quant.Calibrator(tiny['sess'])
    cal.observe(tiny['images'])
    got = cal.finish()
    assert cal.hist_jobs is None and got.method == 'absmax' and got.thresholds is None
    amax, _ = cal.absmax()
    assert got == quant.calibration_from_absmax([[t.name for t in cls] for cls in cal.plan.classes], amax) == quant.calibrate(tiny['sess'], [tiny['images']])
    with pytest.raises(RuntimeError, match='absmax'):
        cal.observe_histogram(tiny['images'])
    cal = quant.Calibrator(tiny['sess'], method='entropy')
    cal.observe(tiny['images'])
    with pytest.raises(RuntimeError, match='second pass'):
        cal.finish()
    with pytest.raises(ValueError, match='method'):
        quant.Calibrator(tiny['sess'], method='median')


def test_histograms_over_other_data_report_their_clamped_count(tiny, caplog):
    from yolo_tf_amd import quant
    cal = quant.Calibrator(tiny['sess'], method='percentile')
    other = torch.from_numpy(np.random.RandomState(3).uniform(0, 255, tuple(tiny['images'].shape)).astype(np.float32)).cuda()
    other[:, 8:24, 8:24] = 255.0
    cal.observe(tiny['images'])
    cal.observe_histogram(other)
    cal.observe_histogram(torch.flip(other, dims=[2]))
    h, clamped = cal.histograms()
    assert clamped.sum() > 0 and (h[:, -1] >= clamped).all()
    with caplog.at_level(logging.WARNING):
        cal.finish()
    assert any('%d values lay above' % int(clamped.sum()) in r.getMessage() for r in caplog.records)


def test_quant_engine_under_an_mse_calibration_equals_the_specification(tiny):
    """The int8 engine with clipped scales: activations saturate at +-127 where the threshold cut, and still equal tests/quant_ref.py bit for bit."""
    from oracle import yolo2_ref as R
    from yolo_tf_amd.session import DetectSession
    calibration = tiny['cal'].finish()
    B, b8 = tiny['B'], tiny['builder8']
    sess8 = DetectSession(b8, B, dtype='int8', seed=5, calibration=calibration)
    sess8.engine.set_variables(tiny['values'])
    sess8.detect(tiny['images'], threshold=0.02, threshold_iou=0.4)
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
    bits = buf[:B * out.h * out.w * ld].view(torch.int16).cpu().numpy().view(np.uint16).reshape(B, out.h, out.w, ld)[..., :out.c]
    nodes = Q.plan(R.SPECS['tiny'](20, 5))
    name_of = {n['out']: op['out'].name for n, op in zip(nodes, b8.graph.ops)}
    params = {k[len('yolo2_tiny') + 1:]: v for k, v in tiny['values'].items()}
    scales = {n: calibration.scales[name_of[n]] for n in Q.int8_tensors(nodes)}
    first = nodes[1]['out']
    spec = Q.run(nodes, params, scales, first, dev[name_of[first]])
    for k, want in spec.items():
        if k not in ('logits', 'logits_bits'):
            assert np.array_equal(dev[name_of[k]], want), k
    assert np.array_equal(bits, spec['logits_bits'])
    clipped = [name for name in calibration.scales if calibration.thresholds[name] < calibration.amax[name]]
    assert clipped and any(int((np.abs(dev[name].astype(np.int32)) == 127).sum()) > 1 for name in clipped)
