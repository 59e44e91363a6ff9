"""Cost of objectness-scaled distillation, three measurements, one process each:

    python scripts/distill_bench.py --kernel                          # the distill launch beside the loss launch on the same buffers, HIP events
    python scripts/distill_bench.py --model darknet                   # bench.py's timed loop (Darknet-19 VOC-20, 416x416, batch 16, bf16, Adam), keys absent
    python scripts/distill_bench.py --model tiny                      # the tiny-20 student alone
    python scripts/distill_bench.py --model tiny --teacher darknet    # ... with a darknet-20 teacher (random weights: the time does not depend on them)

Alternate the configurations in one call (profiles/distill.md has the command).  With YOLO2_LIB_PATH / YOLO2_LIB_BASELINE=1 a run without a teacher takes
the parent commit's library."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step_time(args):
    from bench import make_builder
    from yolo_tf_amd import options
    from yolo_tf_amd.session import DetectSession, TrainSession
    from yolo_tf_amd.utils import data
    base = tempfile.mkdtemp(prefix='distill_bench_')
    builder, cfg = make_builder(args.model, args.names, args.size, True, base)
    kw = {}           # (no teacher: the parent's constructor call, so a baseline library's session builds too)
    if args.teacher:
        tb, _ = make_builder(args.teacher, args.names, args.size, False, os.path.join(base, 'teacher'))
        kw = dict(teacher=DetectSession(tb, args.batch, dtype=args.teacher_dtype, seed=1), distill=dict(class_term=args.class_term, temperature=args.temperature))
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
    fetched = sess.fetch()
    return {'what': 'step', 'model': args.model, 'teacher': args.teacher or None, 'ms_per_step': sorted(windows)[len(windows) // 2], 'windows_ms': windows,
            'steps': args.steps, 'warmup': args.warmup, 'batch': args.batch, 'size': args.size, 'total_loss': fetched['total_loss'], 'distill': fetched.get('distill'),
            'lib': os.environ.get('YOLO2_LIB_PATH') or 'this tree'}


def _timed(fn, reps):
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
    # back to back, one pair of events around all of them: the per-launch time without the events' own barriers
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return {'median_us': sorted(times)[len(times) // 2] * 1e3, 'min_us': min(times) * 1e3, 'back_to_back_us': a.elapsed_time(b) / reps * 1e3}


def kernel_time(args):
    """The distill launch and the loss launch (yolo2_loss_partials) on the same logits and dlogits: 13 x 13 cells, 5 anchors, bf16, ld = pad8."""
    from yolo_tf_amd import ops
    from yolo_tf_amd.utils import data
    out = []
    for batch, classes in ((16, 20), (8, 80)):
        ch = cw = 13
        A, D = 5, 5 * (5 + classes)
        ld = ops.pad8(D)
        gen = torch.Generator(device='cuda').manual_seed(7)
        s = (torch.randn(batch * ch * cw * ld, device='cuda', generator=gen) * 0.7).to(torch.bfloat16)
        t = (torch.randn(batch * ch * cw * ld, device='cuda', generator=gen) * 0.7).to(torch.bfloat16)
        dl = torch.zeros_like(s)
        anchors = torch.tensor([1.08, 1.19, 3.42, 4.41, 6.63, 11.38, 9.42, 5.11, 16.62, 10.52], device='cuda')
        labels = [torch.from_numpy(np.ascontiguousarray(l, np.float32)).cuda() for l in data.synthetic_batch(batch, classes, cw, ch, seed=4321)]
        loss_ws = torch.zeros(ops.loss_ws_floats(batch, ch * cw, A), device='cuda')
        ws = torch.zeros(ops.distill_ws_floats(batch, ch * cw, A), device='cuda')
        row = {'what': 'kernel', 'batch': batch, 'classes': classes, 'lanes': batch * ch * cw * A, 'reps': args.reps,
               'loss': _timed(lambda: ops.loss_partials(s, ld, anchors, labels, [5., 1., 1., 1.], dl, loss_ws, batch, ch, cw, A, classes), args.reps)}
        for term in ('mse', 'kl'):
            row['distill_' + term] = _timed(lambda: ops.distill_partials(s, ld, t, ld, dl, ws, batch, ch, cw, A, classes, class_term=term, temperature=2.0), args.reps)
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernel', action='store_true')
    ap.add_argument('--model', default='darknet', choices=['darknet', 'tiny'])
    ap.add_argument('--teacher', default='', choices=['', 'darknet', 'tiny'])
    ap.add_argument('--teacher_dtype', default='bf16', choices=['bf16', 'f32'])
    ap.add_argument('--class_term', default='mse', choices=['mse', 'kl'])
    ap.add_argument('--temperature', type=float, default=1.0)
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
        raise SystemExit('distill_bench.py measures on the GPU: none is visible')
    for out in (kernel_time(args) if args.kernel else [step_time(args)]):
        out['tag'] = args.tag
        print(json.dumps(out))


if __name__ == '__main__':
    main()
