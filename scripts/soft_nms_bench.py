"""Cost of Soft-NMS (csrc/soft_nms.hip) next to the hard NMS it replaces and the detect batch it is part of (profiles/soft_nms.md; bench.py is
the flagship benchmark and does not cover this).  One process, one call: DetectSession.nms with method hard, linear and gaussian on the SAME
decoded buffers (restored before every launch, outside the timed window), HIP events around the one call, the three methods alternating, the
median and the spread over the repetitions after warm-up.  Darknet-19, 416 x 416, VOC-20, bf16; N = 845, C = 20.  The regimes are those of
scripts/eval_bench.py and bench.py:

  sparse   bench.py's sparse stress input (12 confident boxes per image over a floor below the threshold), batch 256, threshold 0.3 / 0.4
  eval     threshold 0.005 / 0.45 at batch 64, on a detector-like synthetic input (scores 0.9 u^8 with 40 confident boxes per image, the recipe
           of tests/nms_cases.py's eval case) and on the network's own scores for random images (random weights)
  dense    bench.py's dense stress input (scores U(0, 0.5), every box of a class a candidate at 0.3 or not), batch 256, threshold 0.3 / 0.4

For each: the three NMS times, each soft time as a ratio to the hard one and to the whole detect batch (forward + decode + hard NMS, events
around sess.run and sess.nms on the same input), and the candidates per (image, class) that produced them.  Image 0's soft results are
compared with the specification (tests/soft_nms_ref.py) bit for bit.  Prints one JSON line.

The effect of Soft-NMS on the mAP of a trained model is NOT measured here or anywhere in this repository: there is no trained checkpoint
and no dataset."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

METHODS = ('hard', 'linear', 'gaussian')


def eval_like_inputs(batch, classes, seed0):
    import numpy as np
    rng = np.random.RandomState(seed0)
    conf = (rng.uniform(0, 1, (batch, 845, classes)) ** 8 * 0.9).astype(np.float32)
    for b in range(batch):
        hot = rng.choice(845, 40, replace=False)
        conf[b, hot, rng.randint(0, classes, 40)] = rng.uniform(0.3, 0.95, 40).astype(np.float32)
    cen = rng.uniform(0, 13, (batch, 845, 2)).astype(np.float32)
    wh = rng.uniform(0.5, 5.5, (batch, 845, 2)).astype(np.float32)
    return conf, (cen - wh / 2).astype(np.float32), (cen + wh / 2).astype(np.float32)


def summary(x):
    import numpy as np
    x = np.asarray(x, np.float64).reshape(-1)
    return {'min': float(x.min()), 'median': float(np.median(x)), 'mean': float(x.mean()), 'max': float(x.max())}


def measure(args):
    import numpy as np
    import torch
    import bench
    import soft_nms_ref as S
    from yolo_tf_amd.session import DetectSession
    out = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'sigma': args.sigma, 'regimes': {}}
    builder, _ = bench.make_builder('darknet', 20, 416, False, tempfile.mkdtemp())
    regimes = [('sparse', 256, 0.3, 0.4), ('dense', 256, 0.3, 0.4), ('eval_synthetic', 64, 0.005, 0.45), ('eval_network_scores', 64, 0.005, 0.45)]
    sessions = {}
    for name, B, thr, thr_iou in regimes:
        if B not in sessions:
            sessions.clear()                                   # one session at a time: the 256 one holds the larger arena
            sessions[B] = DetectSession(builder, B, dtype='bf16', seed=0)
        sess = sessions[B]
        images = torch.rand(B, 416, 416, 3, device='cuda') * 255.0
        sess.run(images, 0, check_numerics=False)
        if name == 'eval_network_scores':
            for t in (sess.xy_min, sess.xy_max):               # random weights can overflow the box decode: keep the boxes finite
                torch.nan_to_num_(t, nan=0.0, posinf=1e4, neginf=-1e4)
                t.clamp_(-1e4, 1e4)
            saved = [sess.conf.clone(), sess.xy_min.clone(), sess.xy_max.clone()]
        elif name == 'eval_synthetic':
            saved = [torch.from_numpy(a).cuda() for a in eval_like_inputs(B, 20, 2000)]
        else:
            saved = [torch.from_numpy(a).cuda() for a in bench.nms_stress_inputs(name, B, 20, seed0=1000)]

        def restore():
            sess.conf.copy_(saved[0])
            sess.xy_min.copy_(saved[1])
            sess.xy_max.copy_(saved[2])
        K = (saved[0] > thr).sum(dim=1).cpu().numpy()          # candidates per (image, class)
        times = {m: [] for m in METHODS}
        kept = {}
        for rep in range(args.warmup + args.reps):
            for m in METHODS:                                  # alternating: a drift of the machine hits all three alike
                restore()
                a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                sess.nms(thr, thr_iou, method=m, sigma=args.sigma)
                z.record()
                z.synchronize()
                if rep >= args.warmup:
                    times[m].append(a.elapsed_time(z))
                kept[m] = (sess.conf > thr).sum(dim=1).cpu().numpy()
                if rep == 0 and m != 'hard':                   # image 0 against the specification, bit for bit
                    want, _ = S.soft_nms(saved[0][:1].cpu().numpy(), saved[1][:1].cpu().numpy(), saved[2][:1].cpu().numpy(), thr, thr_iou, m, args.sigma)
                    assert np.array_equal(sess.conf[:1].cpu().numpy().view(np.uint32), want.view(np.uint32)), (name, m)
        detect = []
        for rep in range(args.warmup + args.reps):             # the whole detect batch with the hard NMS on this regime's buffers
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            sess.run(images, 0, check_numerics=False)
            restore()
            sess.nms(thr, thr_iou)
            z.record()
            z.synchronize()
            if rep >= args.warmup:
                detect.append(a.elapsed_time(z))
        hard = float(np.median(times['hard']))
        det = float(np.median(detect))
        entry = {'batch': B, 'N': 845, 'C': 20, 'threshold': thr, 'threshold_iou': thr_iou, 'candidates_per_image_class': summary(K),
                 'detect_batch_ms': det, 'checked_against_specification': ['linear', 'gaussian']}
        for m in METHODS:
            t = float(np.median(times[m]))
            entry[m] = {'nms_ms': t, 'min_ms': float(min(times[m])), 'max_ms': float(max(times[m])), 'ratio_to_hard_nms': t / hard,
                        'ratio_to_detect_batch': t / det, 'kept_per_image_class': summary(kept[m])}
        out['regimes'][name] = entry
    sessions.clear()
    out['chain'] = chain(args)
    print(json.dumps(out))


def chain(args):
    """ONE workgroup (B = C = 1) in which every box is a candidate and every pick succeeds (threshold 0, boxes spread out): the launch is
    one serial chain of N picks, so its time over N is the cost of one pick -- one workgroup-wide arg-max and one decay pass over
    ceil(N / 256) positions per thread.  The bytes the launch moves (24 N in, 4 N out) are in the result for comparison."""
    import numpy as np
    import torch
    from yolo_tf_amd import ops
    res = {}
    for N in (256, 1024, 4096):
        rng = np.random.RandomState(N)
        conf = np.linspace(0.01, 0.99, N).astype(np.float32)[rng.permutation(N)].reshape(1, N, 1)
        cen = rng.uniform(0, 40, (1, N, 2)).astype(np.float32)
        wh = rng.uniform(0.5, 5.5, (1, N, 2)).astype(np.float32)
        saved = torch.from_numpy(conf).cuda()
        mn, mx = torch.from_numpy((cen - wh / 2).astype(np.float32)).cuda(), torch.from_numpy((cen + wh / 2).astype(np.float32)).cuda()
        work = saved.clone()
        entry = {}
        for m in ('linear', 'gaussian'):
            t = []
            for rep in range(args.warmup + args.reps):
                work.copy_(saved)
                a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                ops.soft_nms(work, mn, mx, None, 1, N, 1, m, 0.0, 0.45, args.sigma)
                z.record()
                z.synchronize()
                if rep >= args.warmup:
                    t.append(a.elapsed_time(z))
            picks = int((work > 0).sum().item())
            ms = float(np.median(t))
            entry[m] = {'ms': ms, 'picks': picks, 'ns_per_pick': ms * 1e6 / max(picks, 1), 'bytes_moved': 28 * N,
                        'GBps': 28 * N / (ms * 1e-3) / 1e9}
        res[N] = entry
    return res


if __name__ == '__main__':
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--sigma', type=float, default=0.5)
    measure(p.parse_args())
