"""Multi-scale training as train.py runs it, next to fixed-size training (profiles/multiscale.md; bench.py --multiscale cycles the sizes
over random tensors and does not cover the input pipeline or the schedule).  One process: Darknet-19 / VOC-20, bf16, batch 16, a raw-object
.npz of generated 500x375 images that goes through the on-device input pipeline (train.DeviceAugmentedData), config.ini's augmentation.

  1. img/s of `--steps` steps with sizes 320-608 redrawn every 10 steps (multiscale.SizeSchedule + multiscale.follow), of fixed 416x416 and
     of fixed 608x608: wall clock between two device synchronisations, after every size has run once;
  2. the first step at each size against the median of that size's later steps, each step bracketed by synchronisations, in a fresh
     session: what the lazily built plans of a binding cost.  The fixed-size sessions report the same synchronised median.

Every configuration runs in a fresh process of its own, one after the other.  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_dataset(path, n, seed=0):
    import numpy as np
    rng = np.random.RandomState(seed)
    images = rng.randint(0, 256, (n, 375, 500, 3)).astype(np.uint8)
    cls, coord, first = [], [], [0]
    for _ in range(n):
        k = rng.randint(1, 7)
        x0, y0 = rng.uniform(0, 300, k), rng.uniform(0, 225, k)
        cls.append(rng.randint(0, 20, k))
        coord.append(np.stack([x0, y0, x0 + rng.uniform(20, 200, k), y0 + rng.uniform(20, 150, k)], 1))
        first.append(first[-1] + k)
    np.savez(path, images=images, objects_class=np.concatenate(cls).astype(np.int32), objects_coord=np.concatenate(coord).astype(np.float32),
             objects_first=np.asarray(first, np.int32))


def make(args, basedir, path, size, sizes):
    """(session, data) as train.py builds them; ``sizes`` None = the single-size path."""
    import numpy as np
    import train
    from bench import make_builder
    from yolo_tf_amd.session import TrainSession
    builder, cfg = make_builder('darknet', 20, size, True, basedir)
    sess = TrainSession(builder, args.batch, dtype=args.dtype, optimizer='adam', learning_rate=1e-6, seed=0, sizes=sizes)
    data = train.DeviceAugmentedData(np.load(path, allow_pickle=True), args.batch, size, size, 20, size // 32, size // 32, cfg, 0, 0, 1, sess,
                                     sizes=sizes, downsampling=(32, 32) if sizes else None)
    return sess, data


def throughput(args, sess, data, schedule, warm_sizes):
    import torch
    from yolo_tf_amd import multiscale
    for wh in warm_sizes:                           # every size once before the clock starts (plans, filter layouts)
        sess.set_size(*wh)
        sess.step(data.next()[0])
    for _ in range(args.warmup):
        multiscale.follow(sess, schedule, log=Quiet)
        sess.step(data.next()[0])
    torch.cuda.synchronize()
    first = sess.global_step
    t0 = time.perf_counter()
    for _ in range(args.steps):
        multiscale.follow(sess, schedule, log=Quiet)
        sess.step(data.next()[0])
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    data.pipe.check()
    assert sess.fetch()['total_loss'] == sess.fetch()['total_loss'], 'the loss is NaN'
    return {'img_per_s': args.batch * args.steps / elapsed, 'ms_per_step': elapsed / args.steps * 1e3, 'first_global_step': first}


class Quiet(object):
    @staticmethod
    def warning(line):
        pass


def first_steps(args, sess, data, sizes, repeats=6):
    """{WxH: (first step ms, median ms of the following ones)}: synchronised wall clock per step, pipeline included."""
    import numpy as np
    import torch
    out = {}
    for wh in sizes:
        sess.set_size(*wh)
        times = []
        for _ in range(1 + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sess.step(data.next()[0])
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        out['%dx%d' % wh] = {'first_ms': times[0], 'steady_ms': float(np.median(times[1:]))}
    return out


PARTS = ('first_step', 'multiscale', 'fixed_416', 'fixed_608')


def run_part(args, part, basedir, path):
    from yolo_tf_amd import multiscale
    sizes = multiscale.parse_sizes(args.sizes, 32, 32)
    if part == 'first_step':
        sess, data = make(args, basedir, path, 416, sizes)
        return first_steps(args, sess, data, sizes)                                     # (a fresh session: nothing has run at any size yet)
    if part == 'multiscale':
        sess, data = make(args, basedir, path, 416, sizes)
        schedule = multiscale.SizeSchedule(sizes, args.every, 0)
        out = throughput(args, sess, data, schedule, sizes)
        counts = {}
        for g in range(out['first_global_step'], out['first_global_step'] + args.steps):
            counts['%dx%d' % schedule.at(g)] = counts.get('%dx%d' % schedule.at(g), 0) + 1
        out['steps_at'] = counts
        return out
    size = int(part.split('_')[1])
    sess, data = make(args, basedir, path, size, None)
    out = throughput(args, sess, data, None, [])
    # the same synchronised per-step clock as first_step, for a like-for-like figure at this size
    out['synchronised_ms'] = first_steps(args, sess, data, [(size, size)])['%dx%d' % (size, size)]['steady_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--sizes', default='320-608')
    ap.add_argument('--every', type=int, default=10)
    ap.add_argument('--part', default=None, choices=PARTS, help='(internal) run one configuration in this process; --dataset names the .npz')
    ap.add_argument('--dataset', default=None)
    args = ap.parse_args()
    if args.part:
        with tempfile.TemporaryDirectory() as basedir:
            print(json.dumps(run_part(args, args.part, basedir, args.dataset)))
        return
    # One fresh process per configuration, one after the other: a process that has already built and dropped sessions runs a later session's
    # 608x608 steps in 9-10 ms instead of 6 (measured either way round, profiles/multiscale.md), so figures of one process do not compare.
    import subprocess
    from yolo_tf_amd import multiscale
    sizes = multiscale.parse_sizes(args.sizes, 32, 32)
    result = {'metric': 'multiscale_train', 'batch': args.batch, 'dtype': args.dtype, 'steps': args.steps, 'sizes': ['%dx%d' % wh for wh in sizes],
              'every': args.every, 'images': args.images}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'raw.npz')
        write_dataset(path, args.images)
        for part in PARTS:
            cmd = [sys.executable, os.path.abspath(__file__), '--part', part, '--dataset', path] + [a for a in sys.argv[1:]]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError('%s failed (exit %d):\n%s' % (part, r.returncode, r.stderr[-3000:]))
            result[part] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(result))


if __name__ == '__main__':
    main()
