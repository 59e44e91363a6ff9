"""Cost of test-time augmentation (csrc/tta.hip, DetectSession.tta_*) next to the single-view detect batch it multiplies (profiles/tta.md;
bench.py is the flagship benchmark and does not cover this).  One process, one call.  Darknet-19 at 416 x 416, VOC-20, bf16, seeded weights.
Per view set -- {flip}, {320 416 608}, {flip 320 416 608} -- and per regime:

  eval     threshold 0.005 / NMS 0.45 at batch 64: scores 0.9 u^8 with 40 confident boxes per image (the recipe of scripts/soft_nms_bench.py)
  sparse   threshold 0.3 / NMS 0.4 at batch 256: a floor U(0, 0.05) below the threshold and 12 boxes at 0.5 - 0.9 per image (bench.py's sparse input)

the time of detect() at the base size alone, the time of the whole TTA batch (every view: forward, decode, NMS, gather; then fuse and emit), and
the share of the latter spent in gather + fuse + emit, timed on their own on the pooled buffers the batch left.  HIP events, warm-up, the
median over the repetitions, detect and TTA alternating.

Random weights decode to scores that say nothing about a detector, so the decoded tensors are synthetic: every image has 1024 latent boxes
with regime scores; a view's N_v boxes are draws from them, scaled to the view's grid, mirrored for a flipped view, with 1 % jitter on the
coordinates and 10 % on the scores -- the views see the same objects, as views of one image do.  They are copied over the network's decode
inside the timed window (a few MB), so every forward still runs.  Image 0's fused result is compared with the specification bit for bit.

`chain`: ONE workgroup (B = C = 1) walking K candidates: its time over K is the cost of one candidate (IoU against the owned clusters, one
workgroup arg-max, one update), next to the bytes the launch moves.  Prints one JSON line.

The effect of test-time augmentation on the mAP of a trained model is NOT measured here or anywhere in this repository: there is no trained
checkpoint and no dataset."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

VIEW_SETS = ('flip', '320 608', 'flip 320 608')
REGIMES = (('eval', 64, 0.005, 0.45, 1024), ('sparse', 256, 0.3, 0.4, 256))      # name, batch, threshold, NMS overlap, max_per_class
LATENT = 1024


def latent_boxes(regime, B, C, seed):
    import numpy as np
    rng = np.random.RandomState(seed)
    if regime == 'eval':
        conf = (rng.uniform(0, 1, (B, LATENT, C)) ** 8 * 0.9).astype(np.float32)
        hot, lo, hi = 40, 0.3, 0.95
    else:
        conf = rng.uniform(0, 0.05, (B, LATENT, C)).astype(np.float32)
        hot, lo, hi = 12, 0.5, 0.9
    for b in range(B):
        at = rng.choice(LATENT, hot, replace=False)
        conf[b, at, rng.randint(0, C, hot)] = rng.uniform(lo, hi, hot).astype(np.float32)
    cen = rng.uniform(0, 1, (B, LATENT, 2))
    wh = rng.uniform(0.5 / 13, 5.5 / 13, (B, LATENT, 2))
    return conf, cen, wh


def view_boxes(latent, n, cw, ch, flip, seed):
    """(conf [B,n,C], xy_min, xy_max [B,n,2]) f32 in the cells of a (cw, ch) grid."""
    import numpy as np
    conf, cen, wh = latent
    B = conf.shape[0]
    rng = np.random.RandomState(seed)
    idx = rng.randint(0, LATENT, (B, n))
    rows = np.arange(B)[:, None]
    c = cen[rows, idx] + rng.uniform(-0.01, 0.01, (B, n, 2)) * wh[rows, idx]
    s = wh[rows, idx] * rng.uniform(0.99, 1.01, (B, n, 2))
    if flip:
        c[..., 0] = 1.0 - c[..., 0]
    grid = np.array([cw, ch], np.float64)
    sc = (conf[rows, idx] * rng.uniform(0.9, 1.1, (B, n, 1))).astype(np.float32)
    return sc, ((c - s / 2) * grid).astype(np.float32), ((c + s / 2) * grid).astype(np.float32)


def median(x):
    import numpy as np
    return float(np.median(np.asarray(x, np.float64)))


def timed(fn):
    import torch
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    z.record()
    z.synchronize()
    return a.elapsed_time(z)


def measure(args):
    with tempfile.TemporaryDirectory() as basedir:
        _measure(args, basedir)


def _measure(args, basedir):
    import numpy as np
    import torch
    import bench
    import tta_ref as T
    from yolo_tf_amd import ops, tta
    from yolo_tf_amd.session import DetectSession
    out = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'warmup': args.warmup, 'fuse_iou': args.fuse_iou, 'results': []}
    builder, _ = bench.make_builder('darknet', 20, 416, False, basedir)
    for regime, B, thr, thr_iou, per_class in REGIMES:
        latent = latent_boxes(regime, B, 20, 3000)
        for spec in VIEW_SETS:
            views = tta.parse_views(spec, (416, 416), 32, 32)
            sess = DetectSession(builder, B, dtype='bf16', seed=0, tta=views, tta_rows='evaluation' if regime == 'eval' else None)
            images = {wh: torch.rand(B, wh[1], wh[0], 3, device='cuda') * 255.0 for wh in tta.view_sizes(views)}
            decoded = {}
            for v, (w, h, flip) in enumerate(views):
                n = (w // 32) * (h // 32) * sess.A
                decoded[(w, h, flip)] = [torch.from_numpy(a).cuda() for a in view_boxes(latent, n, w // 32, h // 32, flip, 4000 + v)]
            real_run, current = sess.run, [views[0]]

            def run(x, preprocess_mode=0, check_numerics=True):
                real_run(x, preprocess_mode, check_numerics=False)
                for dst, src in zip((sess.conf, sess.xy_min, sess.xy_max), decoded[current[0]]):
                    dst.copy_(src)
                return sess.conf, sess.xy_min, sess.xy_max
            sess.run = run

            def detect_base():
                current[0] = views[0]
                sess.detect(images[(416, 416)], thr, thr_iou)

            def tta_batch():
                sess.tta_begin()
                for view in views:
                    current[0] = view
                    sess.tta_add(images[view[:2]], view, thr, thr_iou)
                sess.tta_fuse(thr, args.fuse_iou, max_per_class=per_class)

            def gathers_only():                                # the V gather launches, from the views' decoded tensors
                for v, view in enumerate(views):
                    c, mn, mx = decoded[view]
                    ops.tta_gather(c, mn, mx, *sess.tta_pooled, B, c.shape[1], sess.C, sess.tta_M, sess._tta_offset[v],
                                   np.float32(13) / np.float32(view[0] // 32), np.float32(13) / np.float32(view[1] // 32), 13.0, view[2])

            def wbf_only():
                ops.wbf(*sess.tta_pooled, *sess.tta_fused, sess.tta_rows, sess.tta_flags, sess.tta_ws, B, sess.tta_M, sess.C, len(views),
                        min(per_class, sess._tta_cap), sess.tta_R, thr, args.fuse_iou)
            t_detect, t_tta, t_gather, t_wbf = [], [], [], []
            for rep in range(args.warmup + args.reps):
                a, b = timed(detect_base), timed(tta_batch)
                if rep >= args.warmup:
                    t_detect.append(a)
                    t_tta.append(b)
            flags = int(sess.tta_flags.item())
            rows = sess.tta_rows.cpu().numpy()
            pooled = [t.clone() for t in sess.tta_pooled]
            K = (pooled[0] > thr).sum(dim=1).cpu().numpy()
            # image 0 against the specification, bit for bit
            want = T.wbf(*[t[:1].cpu().numpy() for t in pooled], thr, args.fuse_iou, len(views), min(per_class, sess._tta_cap), sess.tta_R)
            got = [t[0].cpu().numpy() for t in sess.tta_fused]
            assert int(rows[0]) == int(want[3][0]) and all(np.array_equal(g.view(np.uint32), w[0].view(np.uint32)) for g, w in zip(got, want[:3])), (regime, spec)
            for rep in range(args.warmup + args.reps):
                for dst, src in zip(sess.tta_pooled, pooled):
                    dst.copy_(src)
                b = timed(wbf_only)
                a = timed(gathers_only)
                if rep >= args.warmup:
                    t_gather.append(a)
                    t_wbf.append(b)
            det, whole, g, f = median(t_detect), median(t_tta), median(t_gather), median(t_wbf)
            out['results'].append({
                'regime': regime, 'batch': B, 'threshold': thr, 'threshold_iou': thr_iou, 'views': tta.describe(views), 'V': len(views), 'M': sess.tta_M,
                'R': sess.tta_R, 'max_per_class': min(per_class, sess._tta_cap), 'detect_base_ms': det, 'tta_batch_ms': whole, 'tta_over_detect': whole / det,
                'gather_ms': g, 'fuse_emit_ms': f, 'fusion_share_of_tta': (g + f) / whole, 'tta_min_max_ms': [min(t_tta), max(t_tta)],
                'flags': flags, 'rows_per_image': {'min': int(rows.min()), 'median': float(np.median(rows)), 'max': int(rows.max())},
                'candidates_per_image_class': {'median': float(np.median(K)), 'max': int(K.max())}, 'image0_equals_specification': True})
            del sess
            torch.cuda.empty_cache()
    out['chain'] = chain(args)
    print(json.dumps(out))


def chain(args):
    """B = C = 1, K candidates in groups of sixteen jittered copies (tests/tta_cases.py's recipe): K / 16 or a few more clusters."""
    import numpy as np
    import torch
    import tta_cases
    from yolo_tf_amd import ops
    res = {}
    for K in (256, 1024, 4096):
        rng = np.random.RandomState(K)
        mn, mx = tta_cases._groups(rng, 1, K)
        conf = rng.uniform(0.06, 0.95, (1, K, 1)).astype(np.float32)
        d = [torch.from_numpy(a).cuda() for a in (conf, mn, mx)]
        outs = [torch.zeros(1, K, k, device='cuda') for k in (1, 2, 2)]
        rows, flags = torch.zeros(1, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
        ws = torch.zeros(ops.workspace_bytes('wbf', 1, 1, 1024), dtype=torch.uint8, device='cuda')
        t = []
        for rep in range(args.warmup + args.reps):
            ms = timed(lambda: ops.wbf(*d, *outs, rows, flags, ws, 1, K, 1, 5, 1024, K, 0.05, args.fuse_iou))
            if rep >= args.warmup:
                t.append(ms)
        ms = median(t)
        moved = 24 * K + 20 * int(rows.item()) * 2 + 20 * K
        res[K] = {'ms': ms, 'clusters': int(rows.item()), 'flags': int(flags.item()), 'ns_per_candidate': ms * 1e6 / K, 'bytes_moved': moved,
                  'GBps': moved / (ms * 1e-3) / 1e9}
    return res


if __name__ == '__main__':
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--fuse_iou', type=float, default=0.55)
    measure(p.parse_args())
