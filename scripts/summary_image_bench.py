#!/usr/bin/env python
"""Times one image-summary collection (yolo_tf_amd/summary.py ImageSummaries: the reference's commented `[summary] image` pattern) of a
training session, beside one training step and beside yolo2_histogram over the same tensors, all in one process.

    python scripts/summary_image_bench.py [--inference darknet] [--classes 20] [--size 416] [-b 16] [--dtype bf16] [--reps 20] [--image_max 1 16]

Prints, per image_max: jobs, work items, the bytes the jobs read and write, the device time of collect() (HIP events around the call and
the copy to pinned memory, median of --reps) split into the kernels alone and the copy, the achieved bandwidth, and the host time of
PNG-encoding the result; then the histogram collection of the same pattern (which always reads the whole batch) and the step time."""
import argparse
import configparser
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PATTERN = r'[_\w\d]+\/(input|conv\d*\/(convolution|leaky_relu\/data))$'


def config(**keys):
    c = configparser.ConfigParser()
    c.add_section('summary')
    for k, v in keys.items():
        c.set('summary', k, str(v))
    return c


def device_time(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--inference', default='darknet')
    ap.add_argument('--classes', type=int, default=20)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('-b', '--batch', type=int, default=16)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--image_max', type=int, nargs='+', default=[1, 16])
    args = ap.parse_args()
    from bench import make_builder
    from yolo_tf_amd.session import TrainSession
    from yolo_tf_amd.summary import HistogramSummaries, ImageSummaries
    from yolo_tf_amd.utils import data, png
    b, _ = make_builder(args.inference, args.classes, args.size, True, tempfile.mkdtemp(prefix='summary_image_bench_'))
    sess = TrainSession(b, args.batch, dtype=args.dtype, optimizer='adam', learning_rate=1e-4, seed=1)
    images = torch.rand(args.batch, args.size, args.size, 3, device='cuda') * 255
    labels = data.synthetic_batch(args.batch, args.classes, args.size // 32, args.size // 32, seed=2)
    for _ in range(3):
        sess.step(images, labels)
    torch.cuda.synchronize()
    print('%s-%d %dx%d batch %d %s, pattern %s' % (args.inference, args.classes, args.size, args.size, args.batch, args.dtype, PATTERN))
    step_med, step_min = device_time(lambda: sess.step(images, labels), args.reps)
    print('training step: median %.1f us (min %.1f)' % (step_med, step_min))
    for image_max in args.image_max:
        s = ImageSummaries(sess, config(image=PATTERN, image_max=image_max))
        med, best = device_time(s.collect, args.reps)
        meta, table, host = s._plan()
        kern, kern_best = device_time(table.launch, args.reps)
        read = sum(t.element_size() * rows * c for t, (rows, c, ld) in zip(table.tensors, table.inputs))
        wrote = int(table.out.numel())
        s.collect()
        t0 = time.perf_counter()
        got = s.results()
        t1 = time.perf_counter()
        blobs = [png.encode(g[4]) for g in got]
        t2 = time.perf_counter()
        print('image_max %2d: %4d jobs %6d work items, reads %8.1f MB, result %7.2f MB' % (image_max, table.n, table.items, read / 1e6, wrote / 1e6))
        print('    collect() (call + copy to pinned memory): median %8.1f us (min %8.1f) = %5.2f %% of a step' % (med, best, 100 * med / step_med))
        print('    the four enqueued operations alone:        median %8.1f us (min %8.1f) = %5.2f TB/s of bytes read' % (kern, kern_best, read / kern / 1e6))
        print('    results() after the event (host copy, reshape): %.2f ms;  PNG encoding of %d images, %.2f MB -> %.2f MB: %.1f ms'
              % ((t1 - t0) * 1e3, len(got), sum(g[4].size for g in got) / 1e6, sum(len(x) for x in blobs) / 1e6, (t2 - t1) * 1e3))
    hs = HistogramSummaries(sess, config(histogram=PATTERN))
    med, best = device_time(hs.collect, args.reps)
    tags, table, _ = hs._plan()
    nbytes = sum(t.element_size() * rows * c for t, (rows, c, ld) in zip(table.tensors, table.shapes))
    print('yolo2_histogram, same pattern (whole batch): %d jobs, reads %.1f MB: collect() median %.1f us (min %.1f) = %.2f TB/s = %.2f %% of a step'
          % (len(tags), nbytes / 1e6, med, best, nbytes / med / 1e6, 100 * med / step_med))


if __name__ == '__main__':
    main()
