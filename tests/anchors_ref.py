"""[TF-sem]-style checker of the dimension clusters: the SPECIFICATION in NumPy, not a port (the reference has no such code; its
README.md:88 lists "Dimension cluster" as an open item).  Restates include/yolo2_hip.h, section "dimension clusters": f32 IoU in the
documented operation order, arg-max with ties to the lowest index, exact 64-bit integer sums of fixed-point values, f64 update, bitwise
fixed point detection."""
import numpy as np

_CHUNK = 1 << 16


def iou(boxes, cen):
    """f32 [N][k]: inter = min(w,cw) * min(h,ch); uni = (w*h + cw*ch) - inter; inter / uni, each operation rounded to f32."""
    b = np.asarray(boxes, np.float32)
    c = np.asarray(cen, np.float32)
    w, h = b[:, 0:1], b[:, 1:2]
    cw, ch = c[None, :, 0], c[None, :, 1]
    inter = (np.minimum(w, cw) * np.minimum(h, ch)).astype(np.float32)
    uni = ((w * h).astype(np.float32) + (cw * ch).astype(np.float32)).astype(np.float32) - inter
    out = inter / uni.astype(np.float32)
    assert out.dtype == np.float32
    return out


def assign(boxes, cen):
    """(arg [N] int64, best [N] f32): np.argmax keeps the first of equal values."""
    args, bests = [], []
    for s in range(0, len(boxes), _CHUNK):
        m = iou(boxes[s:s + _CHUNK], cen)
        a = np.argmax(m, axis=1)
        args.append(a)
        bests.append(m[np.arange(len(a)), a])
    return np.concatenate(args), np.concatenate(bests)


def sums(boxes, arg, best, k):
    """(count [k], sum_w [k], sum_h [k]) int64 and the IoU sum as a Python int: rint of the f64 products, added as integers."""
    b = np.asarray(boxes, np.float32).astype(np.float64)
    fw = np.rint(b[:, 0] * 2.0 ** 24).astype(np.int64)
    fh = np.rint(b[:, 1] * 2.0 ** 24).astype(np.int64)
    count, sw, sh = np.zeros(k, np.int64), np.zeros(k, np.int64), np.zeros(k, np.int64)
    np.add.at(count, arg, 1)
    np.add.at(sw, arg, fw)
    np.add.at(sh, arg, fh)
    siou = int(np.sum(np.rint(best.astype(np.float64) * 2.0 ** 30).astype(np.int64), dtype=np.int64))          # < 2^57: exact in int64
    return count, sw, sh, siou


def update(cen, count, sw, sh):
    """New centroids: (float)((double)sum / (double)count * 2^-24); an empty cluster keeps its bits."""
    new = np.array(cen, np.float32, copy=True)
    for c in range(len(new)):
        if count[c] > 0:
            new[c, 0] = np.float32(np.float64(sw[c]) / np.float64(count[c]) * 2.0 ** -24)
            new[c, 1] = np.float32(np.float64(sh[c]) / np.float64(count[c]) * 2.0 ** -24)
    return new


def score(boxes, cen):
    """(avg_iou f64, counts [k] int64, arg [N]) of the centroids as they are."""
    cen = np.asarray(cen, np.float32).reshape(-1, 2)
    arg, best = assign(boxes, cen)
    count, _, _, siou = sums(boxes, arg, best, len(cen))
    return float(siou) / 2.0 ** 30 / float(len(boxes)), count, arg


def step(boxes, cen):
    """One assign + update: (new centroids, counts and avg_iou of the assignment consumed, i.e. of the OLD centroids)."""
    cen = np.asarray(cen, np.float32).reshape(-1, 2)
    arg, best = assign(boxes, cen)
    count, sw, sh, siou = sums(boxes, arg, best, len(cen))
    return update(cen, count, sw, sh), count, float(siou) / 2.0 ** 30 / float(len(boxes)), arg


def fit(boxes, cen, max_iter):
    """Updates until one leaves every centroid bitwise unchanged (that update counts) or max_iter have been applied:
    (centroids, iterations, converged)."""
    cen = np.array(cen, np.float32, copy=True).reshape(-1, 2)
    for it in range(1, max_iter + 1):
        new = step(boxes, cen)[0]
        same = new.view(np.uint32).tolist() == cen.view(np.uint32).tolist()
        cen = new
        if same:
            return cen, it, True
    return cen, max_iter, False
