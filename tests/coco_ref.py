"""Checker of the on-device COCO evaluator: the rules of include/yolo2_hip.h, section "evaluation, COCO protocol" (pycocotools' COCOeval
for boxes, restated), in NumPy with Python loops, written from that text and not from the kernels.  Everything is f64 except the IoU
and the area of a detection, which are f32 in the stated operation order, so that comparisons at a threshold agree bit for bit with the
device."""
import numpy as np

from eval_ref import detections, iou

f32 = np.float32
EPS = 2.220446049250313e-16
AREA_RANGES = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], f32)
IOU_THRESHOLDS = np.linspace(.5, .95, 10).astype(f32)
RECALL_THRESHOLDS = np.linspace(0, 1, 101)
SLICES = [(0, 1), (0, 10), (0, 100), (1, 100), (2, 100), (3, 100)]


def crowd_iou(d, g):
    """Intersection over the DETECTION's area (cell units), f32."""
    d = [f32(v) for v in d]
    g = [f32(v) for v in g]
    w = max(f32(min(d[2], g[2]) - max(d[0], g[0])), f32(0))
    h = max(f32(min(d[3], g[3]) - max(d[1], g[1])), f32(0))
    area = f32(f32(d[2] - d[0]) * f32(d[3] - d[1]))
    return f32(f32(w * h) / max(area, f32(1e-10)))


def det_area(d, scale):
    """Width times height in source pixels: cell extents times pixels per cell, f32."""
    return f32(f32(f32(f32(d[2]) - f32(d[0])) * f32(scale[0])) * f32(f32(f32(d[3]) - f32(d[1])) * f32(scale[1])))


def gt_ignored(area, flags, lo, hi):
    return bool(flags & 3) or bool(f32(area) < lo) or bool(f32(area) > hi)


def match(dets, gts, area_ranges, iou_thresholds):
    """dets: list of (box f32[4], pixel area) in rank order; gts: list of (box, area, flags) of the class in index order.
    Returns (matched, ignored): bool arrays [len(dets), A, T]."""
    A, T = len(area_ranges), len(iou_thresholds)
    matched = np.zeros((len(dets), A, T), bool)
    ignored = np.zeros((len(dets), A, T), bool)
    ious = [[(crowd_iou(d, g) if fl & 2 else iou(d, g)) for g, _, fl in gts] for d, _ in dets]
    for a, (lo, hi) in enumerate(area_ranges):
        ign = [gt_ignored(ar, fl, lo, hi) for _, ar, fl in gts]
        order = [g for g in range(len(gts)) if not ign[g]] + [g for g in range(len(gts)) if ign[g]]      # stable partition
        for t, thr in enumerate(iou_thresholds):
            taken = set()
            for i, (d, area) in enumerate(dets):
                best, m = min(float(thr), 1 - 1e-10), None
                for g in order:
                    if g in taken and not gts[g][2] & 2:
                        continue
                    if m is not None and not ign[m] and ign[g]:
                        break
                    if float(ious[i][g]) < best:
                        continue
                    best, m = float(ious[i][g]), g
                if m is not None:
                    matched[i, a, t] = True
                    ignored[i, a, t] = ign[m]
                    taken.add(m)
                else:
                    ignored[i, a, t] = bool(area < lo) or bool(area > hi)
    return matched, ignored


def collect(conf, xy_min, xy_max, gt_class, gt_box, gt_area, gt_flags, gt_first, scale, image_base, n_valid, threshold, mode,
            area_ranges=AREA_RANGES, iou_thresholds=IOU_THRESHOLDS, max_dets=100):
    """One batch.  Returns (records in emitted order -- image, class, rank --: list of dicts with score, image, box, class, rank,
    matched [A,T], ignored [A,T]; npig [A,C])."""
    B, N, C = conf.shape
    A = len(area_ranges)
    npig = np.zeros((A, C), np.int64)
    records = []
    for b in range(n_valid):
        gts = range(int(gt_first[b]), int(gt_first[b + 1]))
        for g in gts:
            for a, (lo, hi) in enumerate(area_ranges):
                if not gt_ignored(gt_area[g], int(gt_flags[g]), lo, hi):
                    npig[a, gt_class[g]] += 1
        dets = detections(conf[b], threshold, mode)
        for c in sorted(set(d[1] for d in dets)):
            mine = sorted((d for d in dets if d[1] == c), key=lambda d: (-float(d[2]), d[0]))[:max_dets]
            boxes = [np.concatenate([xy_min[b, d[0]], xy_max[b, d[0]]]).astype(f32) for d in mine]
            cls_gts = [(gt_box[g], gt_area[g], int(gt_flags[g])) for g in gts if gt_class[g] == c]
            matched, ignored = match([(bx, det_area(bx, scale[b])) for bx in boxes], cls_gts, area_ranges, iou_thresholds)
            for rank, (box, _, score) in enumerate(mine):
                records.append(dict(score=f32(score), image=image_base + b, box=box, cls=c, rank=rank, matched=matched[rank], ignored=ignored[rank]))
    return records, npig


def bits(flags):
    """[A,T] bools -> the record's bit set (bit a * T + t)."""
    return sum(1 << i for i, v in enumerate(np.asarray(flags).reshape(-1)) if v)


def accumulate(records, npig, C, slices=SLICES, n_iou=len(IOU_THRESHOLDS), recall_thresholds=RECALL_THRESHOLDS):
    """Returns (ap, recall): f64 arrays [S, T, C]."""
    S, T, R = len(slices), n_iou, len(recall_thresholds)
    ap = -np.ones((S, T, C))
    recall = -np.ones((S, T, C))
    for k in range(C):
        mine = sorted((r for r in records if r['cls'] == k), key=lambda r: (-float(r['score']), r['image'], r['rank']))
        for s, (a, limit) in enumerate(slices):
            if npig[a, k] == 0:
                continue
            for t in range(T):
                kept = [r for r in mine if r['rank'] < limit and not r['ignored'][a, t]]
                tp = np.cumsum([1.0 if r['matched'][a, t] else 0.0 for r in kept])
                fp = np.cumsum([0.0 if r['matched'][a, t] else 1.0 for r in kept])
                rc = tp / float(npig[a, k])
                pr = tp / ((fp + tp) + EPS)
                recall[s, t, k] = rc[-1] if len(kept) else 0.0
                for i in range(len(pr) - 1, 0, -1):
                    pr[i - 1] = max(pr[i - 1], pr[i])
                total = 0.0
                for r in recall_thresholds:
                    at = np.nonzero(rc >= r)[0]
                    total += pr[at[0]] if len(at) else 0.0
                ap[s, t, k] = total / R
    return ap, recall


def _mean(x):
    x = x[x > -1]
    return float(np.mean(x)) if x.size else -1.0


def stats(ap, recall, iou_thresholds=IOU_THRESHOLDS):
    """COCO's stats[0..11] for the default six slices (all/1, all/10, all/100, small, medium, large)."""
    def at(t):
        i = np.nonzero(np.asarray(iou_thresholds, f32) == f32(t))[0]
        return _mean(ap[2, i[0]]) if len(i) else -1.0
    return [_mean(ap[2]), at(.5), at(.75), _mean(ap[3]), _mean(ap[4]), _mean(ap[5]),
            _mean(recall[0]), _mean(recall[1]), _mean(recall[2]), _mean(recall[3]), _mean(recall[4]), _mean(recall[5])]


def evaluate(records, npig, C, **kw):
    ap, recall = accumulate(records, npig, C, **kw)
    return dict(ap=ap, recall=recall, stats=stats(ap, recall), npig=npig, detections=len(records))
