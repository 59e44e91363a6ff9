"""Cost of the weight average ([mi355x] ema_decay): bench.py's timed loop (Darknet-19 VOC-20, 416x416, batch 16, bf16, Adam) with the average on or off,
and yolo2_ema_update alone over the Darknet-19 arena (67.16 M parameters, 12 B of traffic each).

    python scripts/ema_bench.py --ema-decay 0        # off: the step bench.py times
    python scripts/ema_bench.py --ema-decay 0.999    # on
    python scripts/ema_bench.py --kernel             # the launch alone, HIP events, median of 50

One process per configuration; alternate them in one call (profiles/ema.md has the command).  With YOLO2_LIB_PATH / YOLO2_LIB_BASELINE=1 the `off` run
takes the parent commit's library."""
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
    builder, cfg = make_builder('darknet', args.names, args.size, True, tempfile.mkdtemp(prefix='ema_bench_'))
    kw = dict(ema_decay=args.ema_decay) if args.ema_decay > 0 else {}       # (off: the parent's constructor call, so a baseline library's session builds too)
    sess = TrainSession(builder, args.batch, dtype=args.dtype, optimizer='adam', learning_rate=1e-6, seed=0, bucket_mb=options.read(cfg, 'bucket_mb'), **kw)
    cells = args.size // 32
    images = torch.rand(args.batch, args.size, args.size, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1234)) * 255.0
    sess.upload_labels(data.synthetic_batch(args.batch, args.names, cells, cells, seed=4321))
    for _ in range(args.warmup):
        sess.step(images)
    torch.cuda.synchronize()
    windows = []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            sess.step(images)
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / args.steps * 1e3)
    loss = sess.fetch()['total_loss']
    return {'what': 'step', 'ema_decay': args.ema_decay, 'ema_arena': sess.ema is not None, 'ms_per_step': sorted(windows)[len(windows) // 2],
            'windows_ms': windows, 'steps': args.steps, 'warmup': args.warmup, 'n_params': sess.engine.n_params, 'total_loss': loss,
            'lib': os.environ.get('YOLO2_LIB_PATH') or 'this tree'}


def kernel_time(args):
    from yolo_tf_amd import ops
    from yolo_tf_amd.engine import staggered
    n = args.n
    w = staggered(n, torch.float32, 'cuda')
    ema = staggered(n, torch.float32, 'cuda')
    w.normal_()
    ema.normal_()
    for _ in range(5):
        ops.ema_update(ema, w, n, 0.001)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.ema_update(ema, w, n, 0.001)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    # back to back, one pair of events around all of them: the per-launch time without the events' own barriers
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        ops.ema_update(ema, w, n, 0.001)
    b.record()
    b.synchronize()
    chain = a.elapsed_time(b) / args.reps
    med = sorted(times)[len(times) // 2]
    return {'what': 'kernel', 'n': n, 'bytes': 12 * n, 'median_ms': med, 'min_ms': min(times), 'back_to_back_ms': chain,
            'TB_per_s_median': 12 * n / med / 1e9, 'TB_per_s_back_to_back': 12 * n / chain / 1e9, 'reps': args.reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ema-decay', type=float, default=0.0)
    ap.add_argument('--kernel', action='store_true')
    ap.add_argument('--n', type=int, default=67160000 // 64 * 64, help='--kernel: elements')
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
        raise SystemExit('ema_bench.py measures on the GPU: none is visible')
    out = kernel_time(args) if args.kernel else step_time(args)
    out['tag'] = args.tag
    print(json.dumps(out))


if __name__ == '__main__':
    main()
