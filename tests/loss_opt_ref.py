"""SPECIFICATION of the loss options of the YOLOv2 loss beyond the box term (csrc/loss_opts.h, csrc/head.hip) -- test
infrastructure, NumPy, generic in dtype like oracle/yolo2_ref.py (float64 for references, float32 to see what the number format costs).  Built on
oracle/yolo2_ref.py (`model_decode`, `objectives`, `loss_backward`) and tests/box_loss_ref.py, which are called as they are; an option that is
off leaves their numbers untouched, so all off IS `R.objectives` / `R.loss_backward`.

Names: mb = mask x "is a best anchor of its cell" (aux['mask_best']); iou = the matching IoU of a lane with its own cell's target; cnt = B cells A.

ignore_thresh = t (0 < t < 1; 0: off).  The ground truth boxes of image b are the object cells of its label tensors (mask != 0), one box per
cell: cell_xy(j) + off_min[j] .. cell_xy(j) + off_max[j] in grid units, area areas[j].  For every lane (b, cell i, anchor a), M = the largest
IoU of its predicted box cell_xy(i) + offset_xy_min .. cell_xy(i) + offset_xy_max with a ground truth box of image b, the one of its own cell
included (0 where the image has none); IoU = inter / max(area_t + area_p - inter, 1e-10), the matching IoU's formula.  A lane with mb == 0 and
M > t (strictly, as Darknet) is ignored: it contributes nothing to `iou_normal` and its dlogits[..., 0] is 0.  Responsible lanes are never
ignored; cnt is not renormalised.

rescore.  The objectness target of a responsible lane is its own matching IoU instead of 1: iou_best = sum(mb (sigma - iou)^2) / cnt and
dlogits[..., 0] uses (sigma - iou) there; iou is a constant in the derivative.  Every other lane's target stays 0.

class_loss = mse | ce | focal, label_smoothing = eps (ce, focal), focal_gamma = gamma (focal; 0 or >= 1).  t = prob[cell], possibly multi-hot,
T = sum_k t_k, tt_k = (1 - eps) t_k + eps T / C.  With p = softmax(class logits) and log p the log-softmax z - max - log sum exp:

    ce      -sum_k tt_k log p_k                           d/dz_j = p_j sum(tt) - tt_j
    focal   -sum_k tt_k (1 - p_k)^gamma log p_k           A_k = tt_k [gamma (1 - p_k)^(gamma - 1) p_k log p_k - (1 - p_k)^gamma],  d/dz_j = A_j - p_j sum_k A_k

times mb and hparam['prob'], over cnt, where the squared error is today; on the responsible lanes only.  focal with gamma = 0 is ce.

`mutation` switches in the mistakes tests/test_loss_opt_cpu.py must see the bounds catch; None is the specification."""
import numpy as np

import box_loss_ref as BS
from oracle import yolo2_ref as R

CLASS_LOSSES = ('mse', 'ce', 'focal')
MUTATIONS = ('other_image', 'no_own_cell', 'ignore_responsible', 'no_cell_xy', 'rescore_grad', 'smooth_c_minus_1', 'focal_half', 'smooth_mse')
DEFAULTS = dict(box_loss='mse', class_loss='mse', ignore_thresh=0.0, rescore=False, label_smoothing=0.0, focal_gamma=2.0)


def max_gt_iou(m, labels, mutation=None):
    """M [B, cells, A] in the dtype of the decode."""
    mask, _, _, tmin, tmax, tareas = labels
    t = m['iou'].dtype.type
    b, cells, a = m['iou'].shape
    cell_xy = R.calc_cell_xy(m['cell_height'], m['cell_width'], m['iou'].dtype).reshape(1, cells, 1, 2)
    if mutation == 'no_cell_xy':
        cell_xy = cell_xy * t(0)
    pmin, pmax = cell_xy + m['offset_xy_min'], cell_xy + m['offset_xy_max']              # [B, cells, A, 2]
    gmin, gmax = (cell_xy + tmin)[:, None, :, 0, :], (cell_xy + tmax)[:, None, :, 0, :]  # [B, 1, cells j, 2]
    garea, gmask = tareas[:, None, :, 0], mask[:, None, :, 0] != 0                        # [B, 1, cells j]
    if mutation == 'other_image':
        gmin, gmax, garea, gmask = (np.roll(x, -1, 0) for x in (gmin, gmax, garea, gmask))
    M = np.zeros((b, cells, a), m['iou'].dtype)
    for k in range(a):       # one anchor at a time: [B, cells i, cells j]
        wh = np.maximum(np.minimum(pmax[:, :, k, None, :], gmax) - np.maximum(pmin[:, :, k, None, :], gmin), t(0))
        inter = wh[..., 0] * wh[..., 1]
        iou = inter / np.maximum(garea + m['areas'][:, :, k, None] - inter, t(1e-10))
        keep = np.broadcast_to(gmask, iou.shape)
        if mutation == 'no_own_cell':
            keep = keep & ~np.eye(cells, dtype=bool)[None]
        M[:, :, k] = np.where(keep, iou, t(0)).max(-1)
    return M


def smoothed(tprob, eps, mutation=None):
    t = tprob.dtype.type
    c = tprob.shape[-1]
    if mutation == 'smooth_c_minus_1':
        return (t(1) - t(eps)) * tprob + t(eps) / t(c - 1)
    return (t(1) - t(eps)) * tprob + t(eps) * tprob.sum(-1, keepdims=True) / t(c)


def class_term(z, tt, class_loss, gamma, mutation=None):
    """(term [..], d term / dz [.., C]) of the ce / focal class loss for class logits z and smoothed targets tt (broadcastable)."""
    t = z.dtype.type
    zm = z - z.max(-1, keepdims=True)
    logp = zm - np.log(np.exp(zm).sum(-1, keepdims=True))
    p = np.exp(logp)
    if class_loss == 'ce' or gamma == 0:
        return -(tt * logp).sum(-1), p * tt.sum(-1, keepdims=True) - tt
    om = t(1) - p
    pw1 = om ** t(gamma - 1)
    pw = pw1 * om
    A = tt * (-pw if mutation == 'focal_half' else t(gamma) * pw1 * (p * logp) - pw)
    return -(tt * pw * logp).sum(-1), A - p * A.sum(-1, keepdims=True)


def loss(net, labels, anchors, hparam, classes, box_loss='mse', class_loss='mse', ignore_thresh=0.0, rescore=False, label_smoothing=0.0,
         focal_gamma=2.0, mutation=None, M=None):
    """net [B, ch, cw, A (5 + C)] -> (objectives dict, aux, dlogits) in net's dtype.  aux adds 'M' (None with the threshold off) and 'ignored'
    (bool [B, cells, A]).  ``M``: a precomputed max_gt_iou of the same inputs."""
    t = net.dtype.type
    assert class_loss in CLASS_LOSSES and (label_smoothing == 0 or class_loss != 'mse' or mutation == 'smooth_mse')
    m = R.model_decode(net, classes, np.asarray(anchors).astype(t), training=True)
    labels = tuple(np.asarray(l).astype(t) for l in labels)
    obj, aux = BS.objectives(m, labels, box_loss)
    dz = BS.loss_backward(m, labels, aux, hparam, classes)
    b, cells, a = m['iou'].shape
    mb, iou, cnt, s = aux['mask_best'], aux['iou'], aux['cnt'], m['iou']
    resp = mb != 0
    ignored = np.zeros(mb.shape, bool)
    aux = dict(aux, M=None)
    dz = dz.reshape(b, cells, a, 5 + classes).copy()
    if ignore_thresh > 0 or rescore:
        if ignore_thresh > 0:
            aux['M'] = max_gt_iou(m, labels, mutation) if M is None or mutation else M
            ignored = (aux['M'] > t(ignore_thresh)) & (True if mutation == 'ignore_responsible' else ~resp)
        tgt = np.where(resp, iou, t(0)) if rescore else mb
        dist = (s - tgt) ** 2
        keep = (~ignored).astype(mb.dtype)
        obj = dict(obj, iou_best=t((keep * mb * dist).sum(dtype=np.float64) / cnt) if mutation == 'ignore_responsible' else t((mb * dist).sum(dtype=np.float64) / cnt),
                   iou_normal=t((keep * (t(1) - mb) * dist).sum(dtype=np.float64) / cnt))
        w_obj = t(hparam['iou_best']) * mb + t(hparam['iou_normal']) * (t(1) - mb)
        dz[..., 0] = keep * (t(2) * (s - tgt) * w_obj / cnt * s * (t(1) - s))
        if rescore and mutation == 'rescore_grad':      # the mistake: d(w_best mb (sigma - iou)^2 / cnt) also through iou(sx, sy, w, h)
            _, _, _, tmin, tmax, tareas = labels
            args = (m['offset_xy'][..., 0], m['offset_xy'][..., 1], m['wh'][..., 0], m['wh'][..., 1], tmin[..., 0], tmin[..., 1], tmax[..., 0], tmax[..., 1], tareas)
            g = BS.score_grad('iou', *args)
            chain = [args[0] * (t(1) - args[0]), args[1] * (t(1) - args[1]), args[2], args[3]]
            for k in range(4):
                dz[..., 1 + k] += np.where(resp, -t(2) * t(hparam['iou_best']) * mb * (s - iou) / cnt * g[k] * chain[k], t(0))
    if class_loss != 'mse' or mutation == 'smooth_mse':
        tprob = labels[1]                                                   # [B, cells, 1, C]
        z = m['inputs'][..., 5:]
        if class_loss == 'mse':                                             # the mistake: the squared error on smoothed targets
            tt = smoothed(tprob, 0.1)
            p = m['prob']
            term = ((p - tt) ** 2).sum(-1)
            d = t(2) * (p - tt)
            grad = p * (d - (d * p).sum(-1, keepdims=True))
        else:
            tt = smoothed(tprob, label_smoothing, mutation)
            term, grad = class_term(z, np.broadcast_to(tt, z.shape), class_loss, focal_gamma, mutation)
        with np.errstate(invalid='ignore'):
            obj = dict(obj, prob=t(np.where(resp, mb * term, t(0)).sum(dtype=np.float64) / cnt))
            dz[..., 5:] = np.where(resp[..., None], (mb * t(hparam['prob']) / cnt)[..., None] * grad, t(0))
    aux['ignored'] = ignored
    return obj, aux, dz.reshape(b, m['cell_height'], m['cell_width'], a * (5 + classes))
