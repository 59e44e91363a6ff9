"""SPECIFICATION of the IoU-family box regression losses of the YOLOv2 loss (`box_loss` = iou, giou, diou, ciou) -- test
infrastructure, NumPy, generic in dtype like oracle/yolo2_ref.py (float64 for references, float32 to see what the number format costs).

Everything except the `coords` objective and channels 1..4 of dlogits is oracle/yolo2_ref.py's `objectives` / `loss_backward`, called as it
is: decode, the matching IoU, the exact-equality choice of responsible anchors, the objectness and class terms.

Frame: the one the matching IoU uses, cell units relative to the cell.  Predicted box P: sx = sigmoid(z1), sy = sigmoid(z2), w = exp(z3) aw,
h = exp(z4) ah, edges sx -+ w/2, sy -+ h/2.  Target T: the labels off_min / off_max, its area the label `areas`.  I, U = max(At + w h - I, 1e-10)
and iou = I / U are formed as `objectives` forms them.  Enclosing box: ew = max(x2, X2) - min(x1, X1), eh likewise.  Score q:

    iou    q = iou
    giou   q = iou - (E - U) / E,          E = max(ew eh, 1e-10)                                   (Rezatofighi et al., CVPR 2019)
    diou   q = iou - rho2 / c2,            rho2 = |(sx, sy) - centre of T|^2, c2 = max(ew^2 + eh^2, 1e-10)   (Zheng et al., AAAI 2020)
    ciou   q = q_diou - alpha v,           v = 4/pi^2 (atan2(Wt, Ht) - atan2(w, h))^2, alpha = v / ((1 - iou) + v + 1e-10)

`coords` = sum(mask_best (1 - q)) / cnt, cnt = B cells A; dlogits[1..4] = d(hparam['coords'] * coords) through sigmoid and exp:
d/dz1 = d/dsx * sx (1 - sx), d/dz3 = d/dw * w; zeros on the lanes that are not responsible.

Conventions at the kinks: at an exact tie of a predicted and a target edge the derivative goes to the predicted edge; max(., 0) and the
1e-10 floors have zero derivative where they clamp.  alpha is a CONSTANT in the derivative, as in the paper; the derivative of v is the
true one, with its 1 / (w^2 + h^2) factor, not the paper's shortcut; w^2 + h^2 is floored at 1e-30 there, which only underflow reaches, so
that a 0 x 0 box leaves dlogits finite (1e-10 would already clamp a 1e-5-cell box, and the factor is the derivative's own).

`score` is written against an array namespace `xp` (numpy or torch) so that tests/test_box_loss_cpu.py can differentiate this very forward
with torch float64 autograd and compare `score_grad`, the hand-derived gradient, against it.  `mutation` switches in the mistakes the mutation
proofs of that test need; None is the specification."""
import math

import numpy as np

from oracle import yolo2_ref as R

METHODS = ('iou', 'giou', 'diou', 'ciou')
MUTATIONS = ('alpha_grad', 'no_w_factor', 'c_not_c2', 'enclose_intersection', 'mask_not_best')
K4 = 4.0 / math.pi ** 2
FLOOR = 1e-10
R2_FLOOR = 1e-30


def _pieces(xp, sx, sy, w, h, X1, Y1, X2, Y2, At, mutation=None):
    x1, x2, y1, y2 = sx - w / 2, sx + w / 2, sy - h / 2, sy + h / 2
    rx = xp.minimum(x2, X2) - xp.maximum(x1, X1)
    ry = xp.minimum(y2, Y2) - xp.maximum(y1, Y1)
    ix, iy = xp.clip(rx, 0, None), xp.clip(ry, 0, None)
    inter = ix * iy
    uraw = At + w * h - inter
    uni = xp.clip(uraw, FLOOR, None)
    if mutation == 'enclose_intersection':
        ew, eh = rx, ry
    else:
        ew = xp.maximum(x2, X2) - xp.minimum(x1, X1)
        eh = xp.maximum(y2, Y2) - xp.minimum(y1, Y1)
    return dict(x1=x1, x2=x2, y1=y1, y2=y2, rx=rx, ry=ry, ix=ix, iy=iy, inter=inter, uraw=uraw, uni=uni, iou=inter / uni, ew=ew, eh=eh)


def score(xp, method, sx, sy, w, h, X1, Y1, X2, Y2, At, mutation=None):
    """q of every lane (arrays of one shape, or broadcastable), with xp = numpy or torch."""
    p = _pieces(xp, sx, sy, w, h, X1, Y1, X2, Y2, At, mutation)
    iou, uni, ew, eh = p['iou'], p['uni'], p['ew'], p['eh']
    if method == 'iou':
        return iou
    if method == 'giou':
        enc = xp.clip(ew * eh, FLOOR, None)
        return iou - (enc - uni) / enc
    dx, dy = sx - (X1 + X2) / 2, sy - (Y1 + Y2) / 2
    rho2 = dx * dx + dy * dy
    c2 = xp.clip(ew * ew + eh * eh, FLOOR, None)
    if mutation == 'c_not_c2':
        c2 = c2 ** 0.5
    q = iou - rho2 / c2
    if method == 'diou':
        return q
    assert method == 'ciou', method
    dth = xp.arctan2(X2 - X1, Y2 - Y1) - xp.arctan2(w, h)
    v = K4 * dth * dth
    alpha = v / ((1 - iou) + v + FLOOR)
    if hasattr(alpha, 'detach') and mutation != 'alpha_grad':
        alpha = alpha.detach()                   # a constant in the derivative
    return q - alpha * v


def score_grad(method, sx, sy, w, h, X1, Y1, X2, Y2, At, mutation=None):
    """The hand-derived (dq/dsx, dq/dsy, dq/dw, dq/dh) in NumPy, in the dtype of the inputs."""
    t = np.asarray(sx).dtype.type
    p = _pieces(np, sx, sy, w, h, X1, Y1, X2, Y2, At, mutation)
    x1, x2, y1, y2, ix, iy, iou, uni, ew, eh = (p[k] for k in ('x1', 'x2', 'y1', 'y2', 'ix', 'iy', 'iou', 'uni', 'ew', 'eh'))
    f = lambda cond: cond.astype(iou.dtype)
    lx, ly = f(p['rx'] > 0), f(p['ry'] > 0)
    ax1, ax2, ay1, ay2 = f(x1 >= X1) * lx, f(x2 <= X2) * lx, f(y1 >= Y1) * ly, f(y2 <= Y2) * ly      # the intersection's edges that are P's
    dI = [iy * (ax2 - ax1), ix * (ay2 - ay1), iy * (ax2 + ax1) / 2, ix * (ay2 + ay1) / 2]              # d/d(sx, sy, w, h)
    uf = f(p['uraw'] > FLOOR)
    dU = [-uf * dI[0], -uf * dI[1], uf * (h - dI[2]), uf * (w - dI[3])]
    g = [(dI[k] - iou * dU[k]) / uni for k in range(4)]
    if method == 'iou':
        return g
    if mutation == 'enclose_intersection':
        bx1, bx2, by1, by2 = f(x1 >= X1), f(x2 <= X2), f(y1 >= Y1), f(y2 <= Y2)
        dew, deh = [bx2 - bx1, 0, (bx2 + bx1) / 2, 0], [0, by2 - by1, 0, (by2 + by1) / 2]
    else:
        bx1, bx2, by1, by2 = f(x1 <= X1), f(x2 >= X2), f(y1 <= Y1), f(y2 >= Y2)                         # the enclosing box's edges that are P's
        dew, deh = [bx2 - bx1, 0, (bx2 + bx1) / 2, 0], [0, by2 - by1, 0, (by2 + by1) / 2]
    if method == 'giou':
        eraw = ew * eh
        enc = np.clip(eraw, FLOOR, None)
        ef = f(eraw > FLOOR)
        return [g[k] + (dU[k] - uni / enc * ef * (eh * dew[k] + ew * deh[k])) / enc for k in range(4)]
    dx, dy = sx - (X1 + X2) / 2, sy - (Y1 + Y2) / 2
    rho2 = dx * dx + dy * dy
    craw = ew * ew + eh * eh
    c2 = np.clip(craw, FLOOR, None)
    cf = f(craw > FLOOR)
    drho = [2 * dx, 2 * dy, 0, 0]
    dc2 = [cf * 2 * (ew * dew[k] + eh * deh[k]) for k in range(4)]
    if mutation == 'c_not_c2':
        dc2 = [d / (2 * c2 ** t(0.5)) for d in dc2]
        c2 = c2 ** t(0.5)
    g = [g[k] - (drho[k] - rho2 / c2 * dc2[k]) / c2 for k in range(4)]
    if method == 'diou':
        return g
    assert method == 'ciou', method
    dth = np.arctan2(X2 - X1, Y2 - Y1) - np.arctan2(w, h)
    v = t(K4) * dth * dth
    den = (1 - iou) + v + t(FLOOR)
    alpha = v / den
    r2 = np.clip(w * w + h * h, t(R2_FLOOR), None)    # a 0 x 0 box (exp underflow) gets a finite, zero, gradient instead of 0 / 0
    dv = [0, 0, -2 * t(K4) * dth * h / r2, 2 * t(K4) * dth * w / r2]
    g = [g[k] - alpha * dv[k] for k in range(4)]
    if mutation == 'alpha_grad':                 # d(alpha v) with alpha = v / den, den = 1 - iou + v + floor, iou differentiated too
        diou = [(dI[k] - iou * dU[k]) / uni for k in range(4)]
        g = [g[k] - v * (dv[k] * den - v * (dv[k] - diou[k])) / (den * den) for k in range(4)]
    return g


def objectives(m, labels, box_loss, mutation=None):
    """As oracle/yolo2_ref.objectives (m: model_decode's dict, labels: the six tensors), with `coords` = sum(mask_best (1 - q)) / cnt.
    Returns (dict of 4 scalars, aux); aux carries what `loss_backward` needs."""
    obj, aux = R.objectives(m, labels)
    if box_loss == 'mse':
        return obj, dict(aux, box_loss='mse')
    mask, _, _, tmin, tmax, tareas = labels
    t = m['iou'].dtype.type
    args = (m['offset_xy'][..., 0], m['offset_xy'][..., 1], m['wh'][..., 0], m['wh'][..., 1],
            tmin[..., 0], tmin[..., 1], tmax[..., 0], tmax[..., 1], tareas)
    q = score(np, box_loss, *args, mutation=mutation)
    sel = (mask * np.ones_like(aux['mask_best'])) if mutation == 'mask_not_best' else aux['mask_best']
    with np.errstate(invalid='ignore'):
        term = np.where(sel != 0, sel * (t(1) - q), t(0))         # only the responsible lanes carry the term (a lane elsewhere may overflow)
    obj = dict(obj, coords=t(term.sum(dtype=np.float64) / aux['cnt']))
    return obj, dict(aux, box_loss=box_loss, box_args=args, box_sel=sel, mutation=mutation)


def loss_backward(m, labels, aux, hparam, classes):
    """As oracle/yolo2_ref.loss_backward: d(total weighted loss)/d net [B, ch, cw, A (5 + C)], channels 1..4 from the box loss of `aux`."""
    dz = R.loss_backward(m, labels, aux, hparam, classes)
    if aux['box_loss'] == 'mse':
        return dz
    t = m['iou'].dtype.type
    b, cells, a = m['iou'].shape
    dz = dz.reshape(b, cells, a, 5 + classes).copy()
    sel, mutation = aux['box_sel'], aux['mutation']
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        g = score_grad(aux['box_loss'], *aux['box_args'], mutation=mutation)
        sx, sy, w, h = aux['box_args'][:4]
        chain = [sx * (t(1) - sx), sy * (t(1) - sy), np.ones_like(w) if mutation == 'no_w_factor' else w, np.ones_like(h) if mutation == 'no_w_factor' else h]
        scale = -(sel * t(hparam['coords']) / aux['cnt'])
        for k in range(4):
            dz[..., 1 + k] = np.where(sel != 0, scale * g[k] * chain[k], t(0))
    return dz.reshape(b, m['cell_height'], m['cell_width'], a * (5 + classes))


def loss(net, labels, anchors, hparam, classes, box_loss, mutation=None):
    """net [B, ch, cw, A (5 + C)] -> (objectives dict, aux, dlogits) in net's dtype."""
    t = net.dtype.type
    m = R.model_decode(net, classes, np.asarray(anchors).astype(t), training=True)
    labels = tuple(np.asarray(l).astype(t) for l in labels)
    obj, aux = objectives(m, labels, box_loss, mutation)
    return obj, aux, loss_backward(m, labels, aux, hparam, classes)
