"""Cost of the loss options ([mi355x] ignore_thresh, rescore, class_loss, label_smoothing, focal_gamma): the loss launch alone
with the options off, each alone and all on, and bench.py's timed loop (Darknet-19 VOC-20, 416x416, batch 16, bf16, Adam) with the keys absent or set.

    python scripts/loss_opt_bench.py --kernel                      # the launch alone at batch 16, C = 20: HIP events, median of 50, and 50 back to back
    python scripts/loss_opt_bench.py --kernel --names 80 --batch 8
    python scripts/loss_opt_bench.py --kernel --dense --batch 16 --size 608    # the worst case: every cell of the 19x19 grid an object
    python scripts/loss_opt_bench.py                               # the training step, keys absent: the step bench.py times
    python scripts/loss_opt_bench.py --options all                 # the training step with every option on

One process per configuration; alternate them in one call (profiles/loss_options.md has the command).  With YOLO2_LIB_PATH / YOLO2_LIB_BASELINE=1 the
run without options takes the parent commit's library (scripts/build_baseline.sh); the kernel run then times the launch with the options off only."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    'off': {},
    'ignore': dict(ignore_thresh=0.6),
    'rescore': dict(rescore=True),
    'ce': dict(class_loss='ce', label_smoothing=0.1),
    'focal': dict(class_loss='focal', label_smoothing=0.1, focal_gamma=2.0),
    'all': dict(box_loss='ciou', ignore_thresh=0.6, rescore=True, class_loss='focal', label_smoothing=0.1, focal_gamma=2.0),
}


def step_time(args):
    from bench import make_builder
    from yolo_tf_amd import options
    from yolo_tf_amd.session import TrainSession
    from yolo_tf_amd.utils import data
    builder, cfg = make_builder('darknet', args.names, args.size, True, tempfile.mkdtemp(prefix='loss_opt_bench_'))
    kw = CONFIGS[args.options]          # (off: the parent's constructor call, so a baseline library's session builds too)
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
    out = sess.fetch()
    return {'what': 'step', 'options': args.options, 'ms_per_step': sorted(windows)[len(windows) // 2], 'windows_ms': windows, 'steps': args.steps,
            'warmup': args.warmup, 'total_loss': out['total_loss'], 'lib': os.environ.get('YOLO2_LIB_PATH') or 'this tree'}


def dense_labels(B, C, cells):
    """Every cell an object: a box of 0.5..3 cells centred in its cell, one class bit."""
    import numpy as np
    from oracle import yolo2_ref as R
    rng = np.random.RandomState(4321)
    outs = []
    for _ in range(B):
        idx = np.arange(cells * cells)
        cx, cy = (idx % cells + rng.uniform(0.2, 0.8, len(idx))) / cells, (idx // cells + rng.uniform(0.2, 0.8, len(idx))) / cells
        w, h = rng.uniform(0.5, 3.0, len(idx)) / cells, rng.uniform(0.5, 3.0, len(idx)) / cells
        outs.append(R.transform_labels(rng.randint(0, C, len(idx)), np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1), C, cells, cells))
    return tuple(np.stack([o[i] for o in outs]) for i in range(6))


def kernel_time(args):
    """The loss launch alone on random logits and labels of bench.py's shape, every configuration in turn."""
    import numpy as np
    from yolo_tf_amd import _lib, ops
    from yolo_tf_amd.utils import data
    B, C, A, cells = args.batch, args.names, 5, args.size // 32
    ld = ops.pad8(A * (5 + C))
    dtype = torch.bfloat16 if args.dtype == 'bf16' else torch.float32
    gen = torch.Generator(device='cuda').manual_seed(7)
    logits = (torch.randn(B, cells * cells, ld, device='cuda', generator=gen) * 0.7).to(dtype)
    dlogits = torch.zeros_like(logits)
    shapes = [(B, cells * cells), (B, cells * cells, C), (B, cells * cells, 4), (B, cells * cells, 2), (B, cells * cells, 2), (B, cells * cells)]
    raw = dense_labels(B, C, cells) if args.dense else data.synthetic_batch(B, C, cells, cells, seed=4321)
    labels = [torch.from_numpy(np.ascontiguousarray(l, np.float32).reshape(s)).cuda() for l, s in zip(raw, shapes)]
    anchors = torch.tensor([1.08, 1.19, 3.42, 4.41, 6.63, 11.38, 9.42, 5.11, 16.62, 10.52], dtype=torch.float32, device='cuda')
    ws = torch.zeros(ops.loss_ws_floats(B, cells * cells, A), dtype=torch.float32, device='cuda')
    hp = [5.0, 1.0, 1.0, 1.0]
    _lib.load()
    rows = {}
    for name, kw in CONFIGS.items():
        if name != 'off' and 'yolo2_loss_ex_partials' in _lib.MISSING:
            continue            # a baseline library: the launch without options only
        launch = lambda: ops.loss_partials(logits, ld, anchors, labels, hp, dlogits, ws, B, cells, cells, A, C, **kw)
        for _ in range(5):
            launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            launch()
        b.record()
        b.synchronize()
        rows[name] = {'median_us': sorted(times)[len(times) // 2], 'min_us': min(times), 'back_to_back_us': a.elapsed_time(b) * 1e3 / args.reps}
    return {'what': 'kernel', 'batch': B, 'classes': C, 'cells': cells, 'dense': bool(args.dense), 'objects': int((labels[0] != 0).sum().item()), 'dtype': args.dtype,
            'reps': args.reps, 'lib': os.environ.get('YOLO2_LIB_PATH') or 'this tree', 'configs': rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--options', default='off', choices=list(CONFIGS))
    ap.add_argument('--kernel', action='store_true')
    ap.add_argument('--dense', action='store_true', help='with --kernel: every cell an object')
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
        raise SystemExit('loss_opt_bench.py measures on the GPU: none is visible')
    out = kernel_time(args) if args.kernel else step_time(args)
    out['tag'] = args.tag
    print(json.dumps(out))


if __name__ == '__main__':
    main()
