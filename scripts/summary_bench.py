#!/usr/bin/env python
"""Times one full histogram collection (yolo_tf_amd/summary.py: every variable, every gradient, every batch moment and every stored activation)
of a training session, against the time the same bytes take at the bandwidth DESIGN.md section 5 measures for adam_filter_prep_kernel.

    python scripts/summary_bench.py [--inference darknet] [--classes 20] [--size 416] [-b 16] [--dtype bf16] [--reps 20]

Prints the per-collection device time (HIP events around the launch and the copy to pinned memory, median of --reps), the bytes the jobs
read, the achieved bandwidth, and the same for three subsets (variables, gradients, activations) to show which kind of tensor costs what."""
import argparse
import configparser
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ADAM_TBPS = 5.72          # adam_filter_prep_kernel, DESIGN.md section 5 (2.15 GB in 376.0 us)


def config(pattern, gradients):
    c = configparser.ConfigParser()
    c.add_section('summary')
    if pattern:
        c.set('summary', 'histogram', pattern)
    c.set('summary', 'gradients', str(int(gradients)))
    return c


def time_collect(hs, reps):
    for _ in range(3):
        hs.collect()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        hs.collect()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    tags, table, _ = hs._plan()
    nbytes = sum(t.element_size() * ((rows - 1) * ld + c if rows and c else 0) for t, (rows, c, ld) in zip(table.tensors, table.shapes))
    return float(np.median(times)), float(np.min(times)), nbytes, len(tags), table.items


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--inference', default='darknet')
    ap.add_argument('--classes', type=int, default=20)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('-b', '--batch', type=int, default=16)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    from bench import make_builder
    from yolo_tf_amd.session import TrainSession
    from yolo_tf_amd.summary import HistogramSummaries
    from yolo_tf_amd.utils import data
    b, _ = make_builder(args.inference, args.classes, args.size, True, tempfile.mkdtemp(prefix='summary_bench_'))
    sess = TrainSession(b, args.batch, dtype=args.dtype, optimizer='adam', learning_rate=1e-4, seed=1)
    images = torch.rand(args.batch, args.size, args.size, 3, device='cuda') * 255
    labels = data.synthetic_batch(args.batch, args.classes, args.size // 32, args.size // 32, seed=2)
    for _ in range(3):
        sess.step(images, labels)
    torch.cuda.synchronize()
    act = r'.*/(input|convolution|leaky_relu/data|BiasAdd|max_pool\d+|reorg|concat\d+)$'
    cases = [('everything', '.*', True), ('variables + moments', r'(?!%s)' % act, False), ('gradients', None, True), ('activations', act, False)]
    print('%s-%d %dx%d batch %d %s' % (args.inference, args.classes, args.size, args.size, args.batch, args.dtype))
    for name, pattern, gradients in cases:
        hs = HistogramSummaries(sess, config(pattern, gradients))
        med, best, nbytes, njobs, items = time_collect(hs, args.reps)
        floor = nbytes / (ADAM_TBPS * 1e12) * 1e6
        print('%-20s %4d jobs %6d work items %9.1f MB: median %8.1f us (min %8.1f) = %5.2f TB/s; the bytes at %.2f TB/s: %6.1f us; ratio %.1f'
              % (name, njobs, items, nbytes / 1e6, med, best, nbytes / med / 1e6, ADAM_TBPS, floor, med / floor))


if __name__ == '__main__':
    main()
