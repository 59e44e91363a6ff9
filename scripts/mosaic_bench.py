"""What mosaic and MixUp cost (profiles/mosaic.md), in one call.

  1. Kernels alone, parameters already on the device: batch 16, 500x375 sources -> 416x416, every colour branch taken (brightness,
     saturation, hue, contrast, noise; no grey, as scripts/augment_bench.py).  yolo2_augment_images' launch pair is timed twice -- the
     difference between the two is the noise floor of this call -- then yolo2_compose_images with one full tile per image (the same
     decisions), with a 2x2 mosaic per image, and with two mosaics blended (MixUp).  The cases alternate, `--rounds` rounds of `--launches`
     launches each between two device events; the figure is the median round.  Achieved bytes per second are against the algorithmic
     bytes: the f32 output once, plus the bytes of each crop's part that shows, once per pass (contrast makes two passes).
  2. The training step as train.py runs it: Darknet-19 / VOC-20, bf16, batch 16, raw objects through the on-device input pipeline with
     config.ini's augmentation, `[mi355x] mosaic = 1` against the key absent; every configuration in a fresh process, alternating, twice.

Prints one JSON line."""
import argparse
import configparser
import ctypes
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, W, H, CLASSES = 16, 416, 416, 20


def kernels(args):
    import numpy as np
    import torch
    from yolo_tf_amd import ops, options
    from yolo_tf_amd.utils import augment as A
    rng = np.random.RandomState(0)
    images = [rng.randint(0, 256, (375, 500, 3)).astype(np.uint8) for _ in range(64)]
    objects = []
    for _ in images:
        k = rng.randint(1, 7)
        x0, y0 = rng.uniform(0, 250, k), rng.uniform(0, 180, k)
        objects.append((rng.randint(0, CLASSES, k), np.stack([x0, y0, x0 + rng.uniform(20, 240, k), y0 + rng.uniform(20, 180, k)], 1)))

    def pipeline(**keys):
        ini = configparser.ConfigParser()          # (a fresh one: the shipped file sets neither mosaic nor mixup)
        ini.read(os.path.join(ROOT, 'config.ini'))
        options.write(ini, argparse.Namespace(**keys), keys)
        cfg = A.AugmentConfig(ini)
        cfg.full_probability = cfg.probability = 1.0          # every branch taken: worst case
        cfg.grayscale_probability = 0.0
        return A.DeviceInputPipeline(images, objects, B, W, H, CLASSES, 13, 13, config=cfg, seed=1)

    up = lambda a: torch.frombuffer(bytearray(bytes(a)), dtype=torch.uint8).cuda()
    plain = pipeline()
    arr = plain.assemble(plain.sample())[0]
    params = up(arr)
    out, ws, src = plain.out, plain.ws, plain.src

    def as_one_tile(arr):
        """The same decisions as a compose call: one full-frame tile per image."""
        from yolo_tf_amd._lib import AugmentParams, ComposeTile
        tiles, photo = (ComposeTile * B)(), (AugmentParams * B)()
        for t, p, a in zip(tiles, photo, arr):
            for f, _ in a._fields_:
                setattr(p, f, getattr(a, f))
            t.src_offset, t.src_w, t.src_h = a.src_offset, a.src_w, a.src_h
            t.crop_x, t.crop_y, t.crop_w, t.crop_h = a.crop_x, a.crop_y, a.crop_w, a.crop_h
            t.view_w, t.view_h, t.x1, t.y1, t.flip = W, H, W, H, int(bool(a.flags & A.FLIP))
        return A.ComposeBatch(tiles, photo, (ctypes.c_float * B)(*([1.0] * B)), 1, 1, None)

    def source_bytes(batch):
        """Bytes of every crop's part that shows in its tile's rectangle, layers whose weight is 0 aside."""
        total = 0.0
        for b in range(B):
            for l in range(batch.L):
                if l == 1 and batch.mix[b] == 1.0:
                    continue
                for k in range(batch.T):
                    t = batch.tiles[(b * batch.L + l) * batch.T + k]
                    w = min(t.x1, t.origin_x + t.view_w) - max(t.x0, t.origin_x)
                    h = min(t.y1, t.origin_y + t.view_h) - max(t.y0, t.origin_y)
                    if w > 0 and h > 0:
                        total += 3.0 * t.crop_w * t.crop_h * (w * h) / (t.view_w * t.view_h)
        return total

    def compose_case(batch):
        dev = (up(batch.tiles), up(batch.photo), up(batch.mix))
        anyc = any(p.flags & A.CONTRAST for p in batch.photo)
        return (lambda: ops.compose_images(src, dev[0], dev[1], dev[2], ws, out, B, batch.L, batch.T, H, W, 114.0, anyc)), source_bytes(batch), dev

    one = as_one_tile(arr)
    mosaic_pipe, mixup_pipe = pipeline(mosaic=1), pipeline(mosaic=1, mixup=1)
    mosaic = mosaic_pipe.assemble(mosaic_pipe.sample())[0]
    mixed = mixup_pipe.assemble(mixup_pipe.sample())[0]
    augment = lambda: ops.augment_images(src, params, ws, out, B, H, W, True)
    plain_bytes = float(sum(3 * a.crop_w * a.crop_h for a in arr))
    cases = [('augment_images', augment, plain_bytes), ('augment_images_again', augment, plain_bytes)]
    keep = []
    for name, batch in (('compose_one_tile', one), ('compose_mosaic', mosaic), ('compose_mosaic_mixup', mixed)):
        fn, nbytes, dev = compose_case(batch)
        keep.append(dev)
        cases.append((name, fn, nbytes))
    # the one-tile compose is the augment launch, bit for bit
    augment()
    want = out.clone()
    cases[2][1]()
    torch.cuda.synchronize()
    assert torch.equal(out, want), 'one full tile does not reproduce yolo2_augment_images'
    for _, fn, _ in cases:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name, _, _ in cases}
    for _ in range(args.rounds):
        for name, fn, _ in cases:
            a.record()
            for _ in range(args.launches):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(e) / args.launches * 1e3)
    out_bytes = B * H * W * 3 * 4
    result = {}
    for name, _, nbytes in cases:
        us = float(np.median(times[name]))
        algorithmic = out_bytes + 2 * nbytes                     # contrast on every image: pass A reads the sources again
        result[name] = {'us': round(us, 2), 'min_us': round(min(times[name]), 2), 'max_us': round(max(times[name]), 2),
                        'algorithmic_MB': round(algorithmic / 1e6, 2), 'TB_per_s': round(algorithmic / us / 1e6, 3)}
    result['noise_floor_us'] = round(abs(result['augment_images']['us'] - result['augment_images_again']['us']), 2)
    # host: the draws and box transforms of a batch
    for name, pipe in (('host_ms_plain', plain), ('host_ms_mosaic', mosaic_pipe), ('host_ms_mosaic_mixup', mixup_pipe)):
        t0 = time.perf_counter()
        for _ in range(20):
            pipe.assemble(pipe.sample())
        result[name] = round((time.perf_counter() - t0) / 20 * 1e3, 3)
    return result


def step(args, mosaic):
    import numpy as np
    import torch
    import train
    from bench import make_builder
    from yolo_tf_amd import options
    from yolo_tf_amd.session import TrainSession
    with tempfile.TemporaryDirectory() as basedir:
        builder, cfg = make_builder('darknet', CLASSES, W, True, basedir)
        if mosaic:
            options.write(cfg, argparse.Namespace(mosaic=1), ['mosaic'])
        sess = TrainSession(builder, B, dtype='bf16', optimizer='adam', learning_rate=1e-6, seed=0)
        data = train.DeviceAugmentedData(np.load(args.dataset, allow_pickle=True), B, W, H, CLASSES, W // 32, H // 32, cfg, 0, 0, 1, sess)
        assert data.pipe.cfg.compose == bool(mosaic)
        for _ in range(args.warmup):
            sess.step(data.next()[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            sess.step(data.next()[0])
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        data.pipe.check()
        loss = sess.fetch()['total_loss']
        assert loss == loss, 'the loss is NaN'
        return {'ms_per_step': round(elapsed / args.steps * 1e3, 3), 'img_per_s': round(B * args.steps / elapsed, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--part', default=None, choices=('kernels', 'step_off', 'step_on'), help='(internal) run one part in this process')
    ap.add_argument('--dataset', default=None)
    args = ap.parse_args()
    if args.part:
        print(json.dumps(kernels(args) if args.part == 'kernels' else step(args, args.part == 'step_on')))
        return
    import subprocess
    from multiscale_train_bench import write_dataset
    result = {'metric': 'mosaic', 'batch': B, 'size': '%dx%d' % (W, H), 'rounds': args.rounds, 'launches': args.launches, 'steps': args.steps}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'raw.npz')
        write_dataset(path, args.images)
        for key, part in (('kernels', 'kernels'), ('step_off_1', 'step_off'), ('step_on_1', 'step_on'), ('step_off_2', 'step_off'), ('step_on_2', 'step_on')):
            cmd = [sys.executable, os.path.abspath(__file__), '--part', part, '--dataset', path] + sys.argv[1:]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError('%s failed (exit %d):\n%s' % (part, r.returncode, r.stderr[-3000:]))
            result[key] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(result))


if __name__ == '__main__':
    main()
