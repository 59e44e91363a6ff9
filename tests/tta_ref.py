"""The specification of yolo2_tta_gather and yolo2_wbf (csrc/tta.hip) in NumPy float32.  Every operation is an IEEE f32 operation on
np.float32 values, one rounding each (no FMA), in the kernels' order, so the kernels' results equal these bit for bit.

A view is (width, height, flip); the base view is the first one and its grid (cell_w0, cell_h0) is the frame of every result.

gather, for a view with grid (cw, ch):  sx = f32(cell_w0) / f32(cw), sy = f32(cell_h0) / f32(ch)  (``scales``: computed once, in f32)

    no flip:  xmin' = xmin * sx                    xmax' = xmax * sx
    flip:     xmin' = f32(cell_w0) - xmax * sx     xmax' = f32(cell_w0) - xmin * sx
    y' = y * sy ; conf is copied

and the views are concatenated along the box axis in view order (M = sum of N_v).

wbf (Weighted Boxes Fusion: Solovyev, Wang, Gabruseva 2021; per class, unit view weights, conf_type = avg), per (image b, class c):

    cand = { i : conf[b, i, c] > threshold }         # NaN and anything <= threshold is no candidate
    for i in cand by (score descending, pooled index ascending):
        iou[k] = inter / max((a_cluster + a_cand) - inter, 1e-10f)   against every cluster's CURRENT FUSED box   (csrc/nms.hip's order)
        k = the first maximum of iou
        if there is a cluster and iou[k] >= fuse_iou:
            Sx0 += s * x0 ; Sy0 += s * y0 ; Sx1 += s * x1 ; Sy1 += s * y1 ; S += s ; T += 1
            fused box = (Sx0 / S, Sy0 / S, Sx1 / S, Sy1 / S)
        else:
            a new cluster: fused box = the candidate's box itself, sums = s * x ..., S = s, T = 1
    score of a cluster = ((S / f32(T)) * f32(min(T, V))) / f32(V)

Per image the clusters are written class ascending, creation order inside a class, into out_conf [B,R,C] (the score in column c, +0.0f
elsewhere), out_xy_min / out_xy_max [B,R,2]; rows[b] = the number of rows written, every later row is +0.0f.  flags: bit 0 = more than
MAX_CANDIDATES candidates in some (image, class), bit 1 = more than max_per_class clusters in some (image, class) -- such an (image, class)
emits nothing -- bit 2 = more than R clusters in an image, which emits its first R.

Boxes are finite with xy_min <= xy_max."""
import numpy as np

F = np.float32
MAX_CANDIDATES = 4096           # YOLO2_WBF_MAX_CANDIDATES (include/yolo2_hip.h)
M_LIMIT = 32768
MAX_PER_CLASS_LIMIT = 1024
FLAG_CANDIDATES, FLAG_CLUSTERS, FLAG_ROWS = 1, 2, 4


def scales(cell_w0, cell_h0, cw, ch):
    """(sx, sy) of a view with grid (cw, ch) in the frame of the base grid: two f32 divisions."""
    return F(cell_w0) / F(cw), F(cell_h0) / F(ch)


def gather_view(conf, xy_min, xy_max, sx, sy, cell_w0, flip):
    """One view's conf [B,N,C], xy_min / xy_max [B,N,2] -> the same in the base frame (new arrays)."""
    mn, mx = np.asarray(xy_min, F), np.asarray(xy_max, F)
    sx, sy, w0 = F(sx), F(sy), F(cell_w0)
    omn, omx = np.empty_like(mn), np.empty_like(mx)
    if flip:
        omn[..., 0] = w0 - mx[..., 0] * sx
        omx[..., 0] = w0 - mn[..., 0] * sx
    else:
        omn[..., 0] = mn[..., 0] * sx
        omx[..., 0] = mx[..., 0] * sx
    omn[..., 1] = mn[..., 1] * sy
    omx[..., 1] = mx[..., 1] * sy
    assert omn.dtype == F and omx.dtype == F
    return np.array(conf, F, copy=True), omn, omx


def gather(views, cell_w0, cell_h0):
    """views: [(conf, xy_min, xy_max, cw, ch, flip)], the base view first -> pooled (conf [B,M,C], xy_min, xy_max [B,M,2])."""
    parts = []
    for conf, mn, mx, cw, ch, flip in views:
        sx, sy = scales(cell_w0, cell_h0, cw, ch)
        parts.append(gather_view(conf, mn, mx, sx, sy, cell_w0, flip))
    return tuple(np.concatenate([p[k] for p in parts], axis=1) for k in range(3))


def check_args(M, C, threshold, fuse_iou, V, max_per_class, R):
    assert 1 <= M <= M_LIMIT and C >= 1
    assert threshold >= 0 and np.isfinite(fuse_iou)
    assert V >= 1 and 1 <= max_per_class <= MAX_PER_CLASS_LIMIT and R >= 1


def iou_clusters(fused, q):
    """IoU of the clusters' fused boxes [n,4] with the candidate box q [4]: the cluster takes the place csrc/nms.hip gives the picked box."""
    a1 = (fused[:, 2] - fused[:, 0]) * (fused[:, 3] - fused[:, 1])
    a2 = (q[2] - q[0]) * (q[3] - q[1])
    w = np.maximum(np.minimum(fused[:, 2], q[2]) - np.maximum(fused[:, 0], q[0]), F(0))
    h = np.maximum(np.minimum(fused[:, 3], q[3]) - np.maximum(fused[:, 1], q[1]), F(0))
    inter = w * h
    return inter / np.maximum((a1 + a2) - inter, F(1e-10))


def wbf_column(s, box, threshold, fuse_iou, V, max_per_class, stats=None):
    """One (image, class): s [M] f32, box [M,4] f32 (xmin, ymin, xmax, ymax) -> (scores [n] f32, boxes [n,4] f32, flags).  An overflow gives
    no clusters and its flag.  stats, if a dict, receives what the walk went through."""
    thr, fiou = F(threshold), F(fuse_iou)
    cand = np.flatnonzero(s > thr)
    if len(cand) > MAX_CANDIDATES:
        return np.zeros(0, F), np.zeros((0, 4), F), FLAG_CANDIDATES
    cand = cand[np.argsort(-s[cand].astype(np.float64), kind='stable')]       # score descending, pooled index ascending
    cap = max_per_class + 1
    fused, sums = np.zeros((cap, 4), F), np.zeros((cap, 4), F)
    S, T = np.zeros(cap, F), np.zeros(cap, np.int64)
    n = joins = 0
    for i in cand:
        sc, q = s[i], box[i]
        k = -1
        if n:
            iou = iou_clusters(fused[:n], q)
            k = int(np.argmax(iou))                        # the first maximum = the lowest cluster index among equals
            if not (iou[k] >= fiou):
                k = -1
        if k >= 0:
            sums[k] = sums[k] + sc * q                     # one multiply and one add per coordinate
            S[k] = S[k] + sc
            T[k] += 1
            fused[k] = sums[k] / S[k]
            joins += 1
        else:
            if n == max_per_class:
                return np.zeros(0, F), np.zeros((0, 4), F), FLAG_CLUSTERS
            fused[n] = q                                   # the box itself: s * x / s does not always round back to x
            sums[n] = sc * q
            S[n], T[n] = sc, 1
            n += 1
    score = ((S[:n] / T[:n].astype(F)) * np.minimum(T[:n], V).astype(F)) / F(V)
    assert score.dtype == F and fused.dtype == F and sums.dtype == F
    if stats is not None:
        stats.update(K=len(cand), clusters=n, joins=joins, T_max=int(T[:n].max()) if n else 0)
    return score, fused[:n].copy(), 0


def wbf(conf, xy_min, xy_max, threshold, fuse_iou, V, max_per_class, R, stats=None):
    """Pooled conf [B,M,C], xy_min / xy_max [B,M,2] -> (out_conf [B,R,C], out_xy_min [B,R,2], out_xy_max [B,R,2], rows [B] int32, flags)."""
    conf, mn, mx = np.asarray(conf, F), np.asarray(xy_min, F), np.asarray(xy_max, F)
    B, M, C = conf.shape
    check_args(M, C, threshold, fuse_iou, V, max_per_class, R)
    out_conf, out_mn, out_mx = np.zeros((B, R, C), F), np.zeros((B, R, 2), F), np.zeros((B, R, 2), F)
    rows, flags = np.zeros(B, np.int32), 0
    with np.errstate(all='ignore'):
        for b in range(B):
            box = np.concatenate([mn[b], mx[b]], axis=1)
            r = 0
            for c in range(C):
                st = None if stats is None else {'b': b, 'c': c}
                score, fused, fl = wbf_column(np.ascontiguousarray(conf[b, :, c]), box, threshold, fuse_iou, V, max_per_class, st)
                if stats is not None:
                    stats.append(st)
                flags |= fl
                for k in range(len(score)):
                    if r == R:
                        flags |= FLAG_ROWS
                        break
                    out_conf[b, r, c] = score[k]
                    out_mn[b, r], out_mx[b, r] = fused[k, :2], fused[k, 2:]
                    r += 1
            rows[b] = r
    return out_conf, out_mn, out_mx, rows, flags
