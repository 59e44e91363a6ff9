"""Checker of the on-device evaluator: the PASCAL VOC devkit rules restated in NumPy (f64, Python loops), written from the rules in
include/yolo2_hip.h, not from the kernels.  Only the IoU is f32, in the reference's operation order (utils/postprocess.py:21-36), so
that comparisons at the threshold agree bit for bit with the device."""
import numpy as np

FP, TP, IGNORED = 0, 1, 2
f32 = np.float32


def iou(a, b):
    """a, b: (xmin, ymin, xmax, ymax) as float32.  (a1 + a2) - inter, floor 1e-10, all in float32."""
    a = [f32(v) for v in a]
    b = [f32(v) for v in b]
    a1 = f32(f32(a[2] - a[0]) * f32(a[3] - a[1]))
    a2 = f32(f32(b[2] - b[0]) * f32(b[3] - b[1]))
    w = max(f32(min(a[2], b[2]) - max(a[0], b[0])), f32(0))
    h = max(f32(min(a[3], b[3]) - max(a[1], b[1])), f32(0))
    inter = f32(w * h)
    return f32(inter / max(f32(f32(a1 + a2) - inter), f32(1e-10)))


def detections(conf, threshold, mode):
    """conf [N,C] of one image -> [(box, class, score)] in (box, class) order."""
    out = []
    if mode == 'detect':
        for i in np.nonzero((conf > threshold).any(1))[0]:
            c = int(np.argmax(conf[i]))
            if conf[i, c] > threshold:
                out.append((int(i), c, f32(conf[i, c])))
    else:
        assert mode == 'all'
        for i, c in zip(*np.nonzero(conf > threshold)):
            out.append((int(i), int(c), f32(conf[i, c])))
    return out


def collect(conf, xy_min, xy_max, gt_class, gt_box, gt_difficult, gt_first, image_base, n_valid, threshold, iou_threshold, mode):
    """One batch.  Returns (records in emitted order: list of (score, class, flag, image, box), npos [C])."""
    B, N, C = conf.shape
    npos = np.zeros(C, np.int64)
    records = []
    for b in range(n_valid):
        gts = list(range(int(gt_first[b]), int(gt_first[b + 1])))
        for g in gts:
            if not gt_difficult[g]:
                npos[gt_class[g]] += 1
        dets = detections(conf[b], threshold, mode)
        flags = {}
        for c in sorted(set(d[1] for d in dets)):
            mine = sorted((d for d in dets if d[1] == c), key=lambda d: (-float(d[2]), d[0]))
            matched = set()
            for box, _, score in mine:
                best, arg = None, None
                for g in gts:
                    if gt_class[g] != c:
                        continue
                    v = iou(np.concatenate([xy_min[b, box], xy_max[b, box]]), gt_box[g])
                    if arg is None or v > best:           # ties stay with the lowest index
                        best, arg = v, g
                flag = FP
                if arg is not None and best > f32(iou_threshold):
                    if gt_difficult[arg]:
                        flag = IGNORED
                    elif arg not in matched:
                        matched.add(arg)
                        flag = TP
                flags[(box, c)] = flag
        for box, c, score in dets:
            records.append((score, c, flags[(box, c)], image_base + b, box))
    return records, npos


def as_arrays(records):
    """list of (score, class, flag, image, box) -> five arrays."""
    if not records:
        return np.zeros(0, f32), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    s, c, f, i, b = zip(*records)
    return np.asarray(s, f32), np.asarray(c, np.int64), np.asarray(f, np.int64), np.asarray(i, np.int64), np.asarray(b, np.int64)


def class_order(score, cls, flag, image, box, c):
    """Indices of the non-ignored records of class c by (score descending, image ascending, box ascending)."""
    idx = np.nonzero((cls == c) & (flag != IGNORED))[0]
    return idx[np.lexsort((box[idx], image[idx], -score[idx].astype(np.float64)))]


def voc_ap(tp, fp, npos):
    """tp, fp: 0/1 arrays along the sorted order.  Returns (ap07, ap12, cumulative tp, cumulative fp); the devkit's VOCevaldet / voc_ap."""
    ctp, cfp = np.cumsum(tp).astype(np.int64), np.cumsum(fp).astype(np.int64)
    if npos == 0:
        return float('nan'), float('nan'), ctp, cfp
    rec = ctp.astype(np.float64) / np.float64(npos)
    prec = ctp.astype(np.float64) / (ctp + cfp).astype(np.float64) if len(ctp) else np.zeros(0)
    ap07 = 0.0
    for k in range(11):
        t = k / 10
        p = prec[rec >= t]
        ap07 += (p.max() if len(p) else 0.0)
    ap07 /= 11
    mrec = np.concatenate([[0.0], rec, [1.0]])
    mpre = np.concatenate([[0.0], prec, [0.0]])
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]          # the monotone envelope: reverse running maximum
    i = np.nonzero(mrec[1:] != mrec[:-1])[0]
    ap12 = float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))
    return float(ap07), ap12, ctp, cfp


def evaluate(records, npos, C):
    """records: list of (score, class, flag, image, box) or the five arrays.  Returns the dictionary Evaluator.result() returns plus
    'order' (per class: the (image, box) pairs in sorted order) and 'cum_tp' / 'cum_fp' (per class)."""
    score, cls, flag, image, box = records if isinstance(records, tuple) else as_arrays(records)
    out = {k: [] for k in ('ap07', 'ap12', 'npos', 'tp', 'fp', 'ignored', 'order', 'cum_tp', 'cum_fp')}
    for c in range(C):
        idx = class_order(score, cls, flag, image, box, c)
        tp = (flag[idx] == TP).astype(np.int64)
        a07, a12, ctp, cfp = voc_ap(tp, 1 - tp, int(npos[c]))
        out['ap07'].append(a07)
        out['ap12'].append(a12)
        out['npos'].append(int(npos[c]))
        out['tp'].append(int(tp.sum()))
        out['fp'].append(int(len(tp) - tp.sum()))
        out['ignored'].append(int(((cls == c) & (flag == IGNORED)).sum()))
        out['order'].append(np.stack([image[idx], box[idx]], 1))
        out['cum_tp'].append(ctp)
        out['cum_fp'].append(cfp)
    for k in ('07', '12'):
        vals = [v for v in out['ap' + k] if not np.isnan(v)]
        out['mAP' + k] = sum(vals) / len(vals) if vals else float('nan')
    out['detections'] = int(len(score))
    return out
