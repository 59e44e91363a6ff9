"""Cost of the on-device evaluator next to the detect batch it scores (profiles/eval_map.md; bench.py is the flagship benchmark and
does not cover this).  One process, HIP events after warm-up:

  1. DetectSession.detect per batch at batch 64 and 256 (Darknet-19, 416x416, VOC-20, bf16) and its NMS launch alone: the baseline;
  2. Evaluator.add per batch on the same batches, both modes, and the host time spent inside add; the same for CocoEvaluator.add
     and for CocoEvaluator.result() on the records of those adds (profiles/eval_coco.md);
  3. Evaluator.result() (the sort and the AP) for M near 1e5 and M = 4952 x 845 synthetic records;
  4. the NumPy checker (tests/eval_ref.py) on the same records, wall time.

``--trace`` instead runs one small evaluation whose window between the first add and result() is bracketed by two back-to-back device
synchronisations, for `rocprofv3 --hip-trace`: the window must hold launches only (scripts/eval_bench.py --analyze trace.csv lists it);
``--protocol coco`` traces the COCO evaluator instead.
Prints one JSON line."""
import argparse
import csv
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def event_ms(fn, reps):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def synthetic_gt(B, classes, cells, seed):
    import numpy as np
    from yolo_tf_amd import evaluate
    rng = np.random.RandomState(seed)
    k = rng.randint(1, 6, B)
    first = np.concatenate([[0], np.cumsum(k)]).astype(np.int32)
    lo = rng.uniform(0, cells - 3, (first[-1], 2))
    box = np.concatenate([lo, lo + rng.uniform(1, 3, (first[-1], 2))], 1).astype(np.float32)
    return evaluate.device_gt(rng.randint(0, classes, first[-1]).astype(np.int32), box, (rng.uniform(size=first[-1]) < 0.1).astype(np.uint8), first)


def coco_gt(gt, B, cells, size):
    """The COCO fields for synthetic_gt's boxes: box area in source pixels, flags = difficult, a square image of `size` pixels."""
    import torch
    cls, box, dif, first = gt
    px = float(size) / cells
    area = (box[:, 2] - box[:, 0]) * px * ((box[:, 3] - box[:, 1]) * px)
    return cls, box, area.contiguous(), dif, first, torch.full((B, 2), px, dtype=torch.float32, device=box.device)


def timed_adds(ev, add, reps):
    """(device ms per add, host microseconds inside add) after three warm-up calls; leaves ONE add in the evaluator."""
    import torch
    for _ in range(3):
        add(0)
    ev.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        add(i)
    host_us = (time.perf_counter() - t0) / reps * 1e6          # no synchronisation inside: this is the enqueue cost
    torch.cuda.synchronize()
    ev.reset()
    it = iter(range(reps))
    ms = event_ms(lambda: add(next(it)), reps)
    return ms, host_us


def synthetic_records(M, C, I, N, seed):
    import numpy as np
    from yolo_tf_amd.evaluate import RECORD_DTYPE
    rng = np.random.RandomState(seed)
    where = rng.permutation(I * N)[:M]
    recs = np.zeros(M, RECORD_DTYPE)
    recs['score'] = rng.uniform(0.005, 1, M).astype(np.float32)
    recs['image'], recs['box'] = where // N, where % N
    cls = rng.randint(0, C, M)
    flag = rng.choice([0, 1, 2], M, p=[0.9, 0.08, 0.02])
    recs['class_flag'] = (cls << 2 | flag).astype(np.uint32)
    npos = np.array([int(((cls == c) & (flag == 1)).sum()) + 100 for c in range(C)], np.int32)
    return recs, cls, flag, npos


def measure(args):
    import numpy as np
    import torch
    import bench
    import eval_ref
    from yolo_tf_amd.evaluate import CocoEvaluator, Evaluator
    from yolo_tf_amd.session import DetectSession
    out = {'device': torch.cuda.get_device_name(0), 'detect': {}, 'add': {}, 'coco_add': {}, 'result': {}}
    builder, _ = bench.make_builder('darknet', 20, 416, False, tempfile.mkdtemp())
    for B in args.batches:
        sess = DetectSession(builder, B, dtype='bf16', seed=0)
        images = torch.rand(B, 416, 416, 3, device='cuda') * 255.0
        thr, thr_iou = args.threshold, 0.45
        for _ in range(3):
            sess.detect(images, thr, thr_iou)
        d = {'detect_ms': event_ms(lambda: sess.detect(images, thr, thr_iou), args.reps)}
        nms = []
        for _ in range(args.reps):                           # NMS zeroes scores in place: decode again before every timed launch
            sess.run(images, check_numerics=False)
            nms.append(event_ms(lambda: sess.nms(thr, thr_iou), 1))
        d['nms_ms'] = float(np.median(nms))
        out['detect'][B] = d
        sess.detect(images, thr, thr_iou)
        gt = synthetic_gt(B, 20, 13, seed=B)
        for mode in ('detect', 'all'):
            ev = Evaluator(20, (args.reps + 4) * B * sess.N * (20 if mode == 'all' else 1), mode=mode, threshold=thr)
            add = lambda: ev.add(sess.conf, sess.xy_min, sess.xy_max, *gt, image_base=0)
            for _ in range(3):
                add()
            ev.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                add()
            host_us = (time.perf_counter() - t0) / args.reps * 1e6          # no synchronisation inside: this is the enqueue cost
            torch.cuda.synchronize()
            ev.reset()
            ms = event_ms(add, args.reps)
            ev.reset()
            add()
            out['add']['%d/%s' % (B, mode)] = {'add_ms': ms, 'host_us_per_add': host_us, 'records': ev.result()['detections']}
            # the COCO evaluator on the same batch, each add a batch of its own (image_base = i * B)
            cgt = coco_gt(gt, B, 13, 416)
            cev = CocoEvaluator(20, (args.reps + 4) * B * 100 * 20, mode=mode, threshold=thr)
            ms, host_us = timed_adds(cev, lambda i: cev.add(sess.conf, sess.xy_min, sess.xy_max, *cgt, image_base=i * B), args.reps)
            res = cev.result()
            torch.cuda.synchronize()
            t = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                res = cev.result()                             # ends in its own synchronisation
                t.append((time.perf_counter() - t0) * 1e3)
            out['coco_add']['%d/%s' % (B, mode)] = {'add_ms': ms, 'host_us_per_add': host_us, 'records_per_add': res['detections'] // args.reps,
                                                   'result_ms': float(np.median(t)), 'records_in_result': res['detections'], 'stats': res['stats']}
        del sess
    for M in ([] if args.skip_results else args.records):
        C, I, N = 20, 4952, 845
        recs, cls, flag, npos = synthetic_records(M, C, I, N, seed=1)
        ev = Evaluator(C, M, mode='all')
        ev.records.copy_(torch.from_numpy(recs.view(np.uint8)).cuda())
        ev.state[0] = M
        ev.npos.copy_(torch.from_numpy(npos).cuda())
        ev.n_images, ev.N = I, N
        res = ev.result()
        torch.cuda.synchronize()
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            res = ev.result()                                 # ends in its own synchronisation
            t.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ref = eval_ref.evaluate((recs['score'], cls.astype(np.int64), flag.astype(np.int64), recs['image'].astype(np.int64), recs['box'].astype(np.int64)),
                                npos, C)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        err = max(abs(a - b) for k in ('ap07', 'ap12') for a, b in zip(res[k], ref[k]))
        assert err <= 1e-9 and res['tp'] == ref['tp'] and res['fp'] == ref['fp']
        out['result'][M] = {'result_ms': float(np.median(t)), 'numpy_checker_ms': numpy_ms, 'max_ap_difference': err}
    print(json.dumps(out))


def trace(args):
    import torch
    import bench
    from yolo_tf_amd.evaluate import CocoEvaluator, Evaluator
    from yolo_tf_amd.session import DetectSession
    B = 64
    builder, _ = bench.make_builder('darknet', 20, 416, False, tempfile.mkdtemp())
    sess = DetectSession(builder, B, dtype='bf16', seed=0)
    sess.detect(torch.rand(B, 416, 416, 3, device='cuda') * 255.0, args.threshold, 0.45)
    gt = synthetic_gt(B, 20, 13, seed=B)
    ev = Evaluator(20, 4 * B * sess.N * 20, mode='all', threshold=args.threshold)
    if args.protocol == 'coco':
        gt = coco_gt(gt, B, 13, 416)
        ev = CocoEvaluator(20, 4 * B * 100 * 20, mode='all', threshold=args.threshold)
    ev.add(sess.conf, sess.xy_min, sess.xy_max, *gt, image_base=0)
    ev.result()                                              # warm-up: allocations and code objects
    ev.reset()
    torch.cuda.synchronize()
    torch.cuda.synchronize()                                 # two in a row: the start of the window in the trace
    for i in range(4):
        ev.add(sess.conf, sess.xy_min, sess.xy_max, *gt, image_base=i * B)
    res = ev.result()
    torch.cuda.synchronize()
    torch.cuda.synchronize()                                 # ... and its end
    print(json.dumps({'detections': res['detections'], 'mAP12': res.get('mAP12'), 'stats': res.get('stats')}))


LAUNCH_CALLS = ('hipLaunchKernel', '__hipPushCallConfiguration', '__hipPopCallConfiguration', 'hipGetLastError')      # one kernel launch = these four


def analyze(path):
    """Lists the HIP API calls between the LAST two pairs of back-to-back hipDeviceSynchronize of a rocprofv3 --hip-trace CSV."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp']))
    names = [r['Function'] for r in rows if r['Function'] not in ('hipGetDevice', 'hipSetDevice')]      # (bookkeeping torch does around every call)
    pairs = [i for i in range(len(names) - 1) if names[i] == names[i + 1] == 'hipDeviceSynchronize']
    assert len(pairs) >= 2, 'window markers not found'
    window = names[pairs[-2] + 2:pairs[-1]]
    counts = {}
    for n in window:
        counts[n] = counts.get(n, 0) + 1
    print(json.dumps({'calls_in_window': counts, 'calls_other_than_launches_in_order': [n for n in window if n not in LAUNCH_CALLS]}))


if __name__ == '__main__':
    p = argparse.ArgumentParser()
    p.add_argument('--batches', type=int, nargs='+', default=[64, 256])
    p.add_argument('--records', type=int, nargs='+', default=[100000, 4952 * 845])
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--threshold', type=float, default=0.005)
    p.add_argument('--trace', action='store_true')
    p.add_argument('--protocol', default='voc', choices=['voc', 'coco'], help='--trace: which evaluator runs inside the window')
    p.add_argument('--skip_results', action='store_true', help='leave out sections 3 and 4 (the VOC sort on synthetic records and its NumPy checker)')
    p.add_argument('--analyze')
    a = p.parse_args()
    if a.analyze:
        analyze(a.analyze)
    elif a.trace:
        trace(a)
    else:
        measure(a)
