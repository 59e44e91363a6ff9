"""The calibration methods of the int8 path on the MI355X, in ONE process (profiles/quant_calibration.md): darknet-20 at 416 x 416, seeded
weights, batches 64 and 256.

  * yolo2_calib_histogram against yolo2_absmax over the same job list (every int8 tensor of the network), alternating the two, each timed
    over enough launches to fill ~50 ms; bytes read per second for both;
  * the cost of one calibration batch in pass 1 (abs-max) and pass 2 (histogram), forward pass included, and the host time of each
    method's threshold selection;
  * relative L2 of the int8 logits against the bf16 logits per method;
  * the histogram launch alone on synthetic bf16 data of three shapes -- spread evenly over the bins, leaky-normal, constant -- which
    separates LDS atomic contention from the loads.

usage: python scripts/calib_bench.py [--out profiles/quant_calibration.md] [--batches 64,256]"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from scripts.quant_bench import time_us

METHODS = ('absmax', 'percentile', 'mse', 'entropy')


def wall_ms(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def measure(B, size=416):
    from bench import make_builder
    from yolo_tf_amd import quant
    from yolo_tf_amd.session import DetectSession
    basedir = tempfile.mkdtemp(prefix='calib_bench_')
    b, _ = make_builder('darknet', 20, size, False, basedir)
    sess = DetectSession(b, B, dtype='bf16', seed=0)
    images = torch.from_numpy(np.random.RandomState(1).uniform(0, 255, (B, size, size, 3)).astype(np.float32)).cuda()
    # timing: one calibrator whose records are thrown away afterwards (repeated launches keep adding to them)
    cal = quant.Calibrator(sess, method='mse')
    pass1_ms = wall_ms(lambda: cal.observe(images))
    pass2_ms = wall_ms(lambda: cal.observe_histogram(images))
    nbytes = sum(cal.engine.B * t.h * t.w * t.c * 2 for t in cal.plan.tensors)
    t = {'absmax': [], 'histogram': []}
    for _ in range(3):              # alternate the two
        t['absmax'].append(time_us(cal.jobs.launch))
        t['histogram'].append(time_us(cal.hist_jobs.launch))
    row = dict(batch=B, tensors=len(cal.plan.tensors), classes=len(cal.plan.classes), bytes=nbytes, absmax_us=min(t['absmax']), hist_us=min(t['histogram']),
               absmax_all=t['absmax'], hist_all=t['histogram'], pass1_ms=pass1_ms, pass2_ms=pass2_ms)
    del cal
    torch.cuda.empty_cache()
    # accuracy: a fresh calibrator, each pass once
    cal = quant.Calibrator(sess, method='mse')
    cal.observe(images)
    cal.observe_histogram(images)
    h, clamped = cal.histograms()
    assert not clamped.any()
    amax, _ = cal.absmax()
    classes = [[x.name for x in cls] for cls in cal.plan.classes]
    sess.run(images, check_numerics=False)
    out = sess.engine.output()
    n = B * out.h * out.w * sess.engine.act[out][1]
    ref = sess.engine.act[out][0][:n].float().cpu().numpy().astype(np.float64)
    variables = sess.engine.get_variables()
    limits = cal.limits
    del cal
    torch.cuda.empty_cache()
    for method in METHODS:
        t0 = time.perf_counter()
        if method == 'absmax':
            calibration = quant.calibration_from_absmax(classes, amax)
        else:
            calibration, report = quant.calibration_from_histograms(classes, limits, h, method, 99.99)
            row[method + '_ratio'] = float(np.mean([r['threshold'] / r['amax'] for r in report]))
        row[method + '_host_ms'] = (time.perf_counter() - t0) * 1e3
        b8, _ = make_builder('darknet', 20, size, False, basedir)
        sess8 = DetectSession(b8, B, dtype='int8', seed=0, calibration=calibration)
        sess8.engine.set_variables(variables)
        sess8.run(images, check_numerics=False)
        got = sess8.engine.act[sess8.engine.output()][0][:n].float().cpu().numpy().astype(np.float64)
        row[method + '_rel'] = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        del sess8
        torch.cuda.empty_cache()
    print(row, flush=True)
    return row


def contention(jobs=16, n=1 << 24):
    """16 jobs of 2^24 bf16 values in one slot (512 MiB): the same bytes, three distributions over the bins."""
    from yolo_tf_amd import ops
    rows = []
    gen = torch.Generator(device='cuda').manual_seed(0)
    for name in ('uniform over the bins', 'leaky normal, limit = abs-max', 'constant'):
        if name.startswith('uniform'):
            x = torch.rand(jobs * n, device='cuda', generator=gen)
        elif name.startswith('leaky'):
            x = torch.randn(jobs * n, device='cuda', generator=gen)
            x = torch.where(x > 0, x, x * 0.1)
        else:
            x = torch.full((jobs * n,), 0.3, device='cuda')
        x = x.to(torch.bfloat16)
        limit = float(x.float().abs().max())
        table = ops.CalibHistogramJobs([(x[j * n:], 1, n, n, 0, limit) for j in range(jobs)], 1)
        table.launch()
        h, _, _ = table.result()
        assert int(h.sum()) == jobs * n
        top = float(np.sort(h[0])[::-1][:BINS_TENTH].sum()) / float(h.sum())
        us = min(time_us(table.launch) for _ in range(3))
        rows.append(dict(name=name, bytes=jobs * n * 2, us=us, top=top))
        print(rows[-1], flush=True)
        del x, table
        torch.cuda.empty_cache()
    return rows


BINS_TENTH = 205


def report(rows, probe):
    lines = ['# int8 calibration methods on the MI355X (scripts/calib_bench.py)', '',
             'darknet-20 at 416 x 416, seeded weights, one process.  The two launches read the same job list: every int8 tensor of the network',
             'as the calibrator\'s engine stores it (bf16, pools un-fused).  Times are the best of three alternating windows of ~50 ms each.', '',
             '| batch | tensors / scale classes | bytes read | `yolo2_absmax` us | TB/s | `yolo2_calib_histogram` us | TB/s | histogram / abs-max time |',
             '|---|---|---|---|---|---|---|---|']
    for r in rows:
        lines.append('| %d | %d / %d | %d | %.1f | %.2f | %.1f | %.2f | %.2f |' % (
            r['batch'], r['tensors'], r['classes'], r['bytes'], r['absmax_us'], r['bytes'] / r['absmax_us'] * 1e-6, r['hist_us'],
            r['bytes'] / r['hist_us'] * 1e-6, r['hist_us'] / r['absmax_us']))
    lines += ['', 'All windows, us: ' + '; '.join('batch %d abs-max %s, histogram %s' % (
        r['batch'], ' '.join('%.1f' % v for v in r['absmax_all']), ' '.join('%.1f' % v for v in r['hist_all'])) for r in rows), '',
        'One calibration batch (forward pass of the un-fused bf16 engine plus the launch, wall clock with a synchronisation, mean of 3) and the',
        'host time of choosing every class\'s threshold once, after the last batch:', '',
        '| batch | pass 1 (abs-max) ms | pass 2 (histogram) ms | `absmax` per batch | other methods per batch | host: percentile ms | mse ms | entropy ms |',
        '|---|---|---|---|---|---|---|---|']
    for r in rows:
        lines.append('| %d | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f |' % (
            r['batch'], r['pass1_ms'], r['pass2_ms'], r['pass1_ms'], r['pass1_ms'] + r['pass2_ms'], r['percentile_host_ms'], r['mse_host_ms'],
            r['entropy_host_ms']))
    lines += ['', 'Relative L2 of the int8 logits against the bf16 logits, calibrated on the evaluated batch (percentile 99.99); in brackets the mean',
              'threshold / abs-max over the scale classes:', '', '| batch | absmax | percentile | mse | entropy |', '|---|---|---|---|---|']
    for r in rows:
        lines.append('| %d | %.4f | %.4f (%.3f) | %.4f (%.3f) | %.4f (%.3f) |' % (
            r['batch'], r['absmax_rel'], r['percentile_rel'], r['percentile_ratio'], r['mse_rel'], r['mse_ratio'], r['entropy_rel'], r['entropy_ratio']))
    lines += ['', 'The histogram launch alone on synthetic bf16 data, 16 jobs of 2^24 values in one slot (the same 512 MiB each time):', '',
              '| values | share of the counts in the fullest tenth of the bins | us | TB/s |', '|---|---|---|---|']
    for r in probe:
        lines.append('| %s | %.3f | %.1f | %.2f |' % (r['name'], r['top'], r['us'], r['bytes'] / r['us'] * 1e-6))
    return '\n'.join(lines) + '\n'


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--batches', default='64,256')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the measurement needs the GPU'
    text = report([measure(int(b)) for b in args.batches.split(',')], contention())
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
