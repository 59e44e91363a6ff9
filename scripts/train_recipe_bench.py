"""Cost of the training recipe of DESIGN.md section 23 ([mi355x] accum_steps, weight_decay): bench.py's timed loop (Darknet-19 VOC-20, 416x416, batch 16,
bf16, Adam) with the keys absent, with weight_decay = 5e-4 at K = 1, and the micro-step at K = 4; and yolo2_grad_combine's ADD and FINAL launches alone over
the Darknet-19 arena beside yolo2_ema_update from the same process.

    python scripts/train_recipe_bench.py                                  # keys absent: the step bench.py times
    python scripts/train_recipe_bench.py --weight-decay 5e-4              # K = 1, the FINAL launch with the L2 term in front of Adam
    python scripts/train_recipe_bench.py --accum-steps 4                  # ms per MICRO-step (one update every fourth)
    python scripts/train_recipe_bench.py --kernel                         # the launches alone, HIP events

One process per configuration; alternate them in one call (profiles/train_recipe.md has the command).  With YOLO2_LIB_PATH / YOLO2_LIB_BASELINE=1 the
keys-absent run takes the parent commit's library (scripts/build_baseline.sh)."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step_time(args):
    from bench import make_builder
    from yolo_tf_amd import options
    from yolo_tf_amd.session import TrainSession
    from yolo_tf_amd.utils import data
    builder, cfg = make_builder('darknet', args.names, args.size, True, tempfile.mkdtemp(prefix='train_recipe_bench_'))
    kw = {}                                  # (keys absent: the parent's constructor call)
    if args.accum_steps > 1:
        kw['accum_steps'] = args.accum_steps
    if args.weight_decay > 0:
        kw.update(weight_decay=args.weight_decay, weight_decay_mode=args.weight_decay_mode)
    sess = TrainSession(builder, args.batch, dtype=args.dtype, optimizer='adam', learning_rate=1e-6, seed=0, bucket_mb=options.read(cfg, 'bucket_mb'), **kw)
    cells = args.size // 32
    images = torch.rand(args.batch, args.size, args.size, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1234)) * 255.0
    sess.upload_labels(data.synthetic_batch(args.batch, args.names, cells, cells, seed=4321))
    K = max(1, args.accum_steps)
    steps, warmup = args.steps // K * K, (args.warmup + K - 1) // K * K          # whole updates
    for _ in range(warmup):
        sess.step(images)
    torch.cuda.synchronize()
    windows = []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        for _ in range(steps):
            sess.step(images)
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / steps * 1e3)
    loss = sess.fetch()['total_loss']
    return {'what': 'step', 'accum_steps': K, 'weight_decay': args.weight_decay, 'weight_decay_mode': args.weight_decay_mode if args.weight_decay > 0 else None,
            'ms_per_micro_step': sorted(windows)[len(windows) // 2], 'windows_ms': windows, 'steps': steps, 'warmup': warmup, 'updates': sess.global_step,
            'n_params': sess.engine.n_params, 'total_loss': loss, 'lib': os.environ.get('YOLO2_LIB_PATH') or 'this tree'}


def _time(fn, reps):
    """(median of `reps` event-bracketed launches, the fastest, `reps` launches back to back under one event pair) in ms."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return sorted(times)[len(times) // 2], min(times), a.elapsed_time(b) / reps


def kernel_time(args):
    """The arenas of a Darknet-19 session (its own layout, so the decayed ranges are the real ones); values small enough that 150 ADDs stay finite."""
    from bench import make_builder
    from yolo_tf_amd import ops
    from yolo_tf_amd.engine import layout_params, staggered
    from yolo_tf_amd.session import decay_ranges
    builder, _ = make_builder('darknet', args.names, args.size, True, tempfile.mkdtemp(prefix='train_recipe_bench_'))
    offsets, n = layout_params(builder.graph)
    ranges = decay_ranges(offsets)
    table = ops.grad_ranges(ranges, n, 'cuda')
    decayed = sum(e - b for b, e in ranges)
    g, acc, w, ema = [staggered(n, torch.float32, 'cuda') for _ in range(4)]
    for t in (g, acc, w, ema):
        t.normal_(std=1e-3)
    shrink = 1.0 - 1e-3 * 5e-4
    launches = [
        ('ema_update', 12 * n, lambda: ops.ema_update(ema, w, n, 0.001)),
        ('grad_combine STORE', 8 * n, lambda: ops.grad_combine(g, acc, None, n, ops.GRAD_STORE)),
        ('grad_combine ADD', 12 * n, lambda: ops.grad_combine(g, acc, None, n, ops.GRAD_ADD)),
        ('grad_combine FINAL acc', 12 * n, lambda: ops.grad_combine(g, acc, None, n, ops.GRAD_FINAL, 0.25)),
        ('grad_combine FINAL acc + l2', 12 * n + 4 * decayed, lambda: ops.grad_combine(g, acc, w, n, ops.GRAD_FINAL, 0.25, 5e-4, 1.0, table)),
        ('grad_combine FINAL acc + decoupled', 12 * n + 8 * decayed, lambda: ops.grad_combine(g, acc, w, n, ops.GRAD_FINAL, 0.25, 0.0, shrink, table)),
        ('grad_combine FINAL l2, no acc', 8 * n + 4 * decayed, lambda: ops.grad_combine(g, None, w, n, ops.GRAD_FINAL, 1.0, 5e-4, 1.0, table)),
        ('ema_update again', 12 * n, lambda: ops.ema_update(ema, w, n, 0.001)),
    ]
    rows = []
    for name, nbytes, fn in launches:
        med, fastest, chain = _time(fn, args.reps)
        rows.append({'launch': name, 'bytes': nbytes, 'median_us': med * 1e3, 'min_us': fastest * 1e3, 'back_to_back_us': chain * 1e3,
                     'TB_per_s_median': nbytes / med / 1e9, 'TB_per_s_back_to_back': nbytes / chain / 1e9})
    return {'what': 'kernel', 'n': n, 'decayed': decayed, 'ranges': len(ranges), 'reps': args.reps, 'launches': rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--accum-steps', type=int, default=1)
    ap.add_argument('--weight-decay', type=float, default=0.0)
    ap.add_argument('--weight-decay-mode', default='l2', choices=['l2', 'decoupled'])
    ap.add_argument('--kernel', action='store_true')
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--windows', type=int, default=3, help='timed windows of --steps steps; the median is reported')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--names', type=int, default=20, choices=[20, 80])
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'f32'])
    ap.add_argument('--tag', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('train_recipe_bench.py measures on the GPU: none is visible')
    out = kernel_time(args) if args.kernel else step_time(args)
    out['tag'] = args.tag
    print(json.dumps(out))


if __name__ == '__main__':
    main()
