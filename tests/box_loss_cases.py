"""Cases, float64 references and bounds for the IoU-family box losses (tests/box_loss_ref.py is the specification; csrc/box_loss.h and
csrc/head.hip the kernel).  tests/test_box_loss_cpu.py checks the cases themselves and proves that the bounds catch wrong losses;
tests/test_box_loss_gpu.py launches the kernel on them.

Cases: the thirteen geometries of head_cases.V2_SPECS, in the modes each lists (their no-near-tie property for the matching is proven in
tests/test_head_cases_cpu.py), plus three placed ones on a 7x10 grid, B = 2, A = 5, C = 4, five objects per image:

    disjoint   0.3-cell targets centred at 0.2 / 0.8 of the cell, every anchor predicting a 0.15..0.35-cell box centred at sigmoid(+-1.5) in the
               opposite corner: IoU exactly 0 for all five anchors, all five responsible.  The iou mode's box gradient is exactly zero;
               GIoU, DIoU and CIoU still pull.
    inside     targets of 2..4 cells, predictions 0.1 cells off the target's centre and 0.8 / 0.6 / 0.5 / 0.4 / 0.3 of its size: inside the
               target, so GIoU equals IoU and IoU has no centre gradient; DIoU has one.
    encloses   targets of 1..2 cells, predictions 0.05 cells off the centre and 1.25 .. 3 times the target's size.

In `inside` and `encloses` every prediction is 1.1 times wider and 1.1 times lower than its scale says (or the reverse, alternating with
the object), so the winning anchor's aspect ratio differs from the target's by 21 % and CIoU's term is live.

Bounds: head_cases.f32_ratio (f32 dlogits), bf16_ratio (bf16 dlogits), objective_ratio (objectives); 1.0 is the bound.  `tie_all` is kept for the
objectives and for "no NaN": its box gradients are below 1e-7 (saturated sigmoids, 1e-4-cell boxes), where s (1 - s) in float32 alone costs
more than 1e-4 relative, so the float32 specification itself is not within 0.25 of the gradient bound there (GRADIENT_CONDITION_EXEMPT)."""
import functools

import numpy as np

import box_loss_ref as S
import head_cases as H
from oracle import yolo2_ref as R

METHODS = S.METHODS
PLACED_SPECS = {
    'disjoint': (2, 7, 10, 5, 4, None, 'disjoint', 41, H.MODES),
    'inside':   (2, 7, 10, 5, 4, None, 'inside', 42, H.MODES),
    'encloses': (2, 7, 10, 5, 4, None, 'encloses', 43, H.MODES),
}
CASES = list(H.V2_SPECS) + list(PLACED_SPECS)             # (no reused case broke a condition: none is dropped, none has a new seed)
GRADIENT_CONDITION_EXEMPT = ('tie_all',)
ASPECT = 1.1
KINK = 1e-5                                                # every responsible lane is at least this far (cells) from every kink
F32_SELF = 0.25                                            # the float32 specification against its float64 self: this share of a bound


def modes(name):
    return (H.V2_SPECS.get(name) or PLACED_SPECS[name])[8]


ALL = [(n, m, k) for n in CASES for m in modes(n) for k in METHODS]


@functools.lru_cache(maxsize=None)
def case(name):
    """head_cases.v2_case's dict (see there) for a reused or a placed case; callers must not write to it."""
    if name in H.V2_SPECS:
        return H.v2_case(name)
    B, ch, cw, A, C, ld, recipe, seed, case_modes = PLACED_SPECS[name]
    rng = np.random.RandomState(seed)
    d, cells = 5 + C, ch * cw
    anchors = H.VOC_ANCHORS[:A].copy()
    net = rng.randn(B, cells, A, d) * 0.7
    if recipe == 'disjoint':
        corner = lambda r: tuple(r.choice([0.2, 0.8], 2))
        labels, idx, offs, sizes = H._placed_labels(rng, B, C, cw, ch, 5, corner, lambda r: (0.3, 0.3))
    elif recipe == 'inside':
        labels, idx, offs, sizes = H._placed_labels(rng, B, C, cw, ch, 5, lambda r: tuple(r.uniform(0.25, 0.75, 2)), lambda r: tuple(r.uniform(2.0, 4.0, 2)))
    else:
        labels, idx, offs, sizes = H._placed_labels(rng, B, C, cw, ch, 5, lambda r: tuple(r.uniform(0.25, 0.75, 2)), lambda r: tuple(r.uniform(1.0, 2.0, 2)))
    resp = np.zeros((B, cells), np.int64)
    for b in range(B):
        for j, (i, o, s) in enumerate(zip(idx[b], offs[b], sizes[b])):
            if recipe == 'disjoint':
                net[b, i, :, 1:3] = np.where(o < 0.5, 1.5, -1.5)
                size = rng.uniform(0.15, 0.35, (A, 2))
                resp[b, i] = A
            else:
                scale = np.array([0.8, 0.6, 0.5, 0.4, 0.3]) if recipe == 'inside' else np.array([1.25, 1.6, 2.0, 2.5, 3.0])
                net[b, i, :, 1:3] = H._logit(o + (0.1 if recipe == 'inside' else 0.05))
                aspect = np.array([ASPECT, 1 / ASPECT]) if j % 2 == 0 else np.array([1 / ASPECT, ASPECT])
                size = s[None, :] * scale[:, None] * aspect[None, :]
                resp[b, i] = 1
            net[b, i, :, 3:5] = np.log(size / anchors.astype(np.float64))
    D = A * d
    net = net.reshape(B, ch, cw, D).astype(np.float32)
    net.setflags(write=False)
    return dict(name=name, B=B, ch=ch, cw=cw, A=A, C=C, D=D, ld=ld or H.pad8(D), net=net, anchors=anchors, labels=labels, modes=case_modes, resp=resp)


@functools.lru_cache(maxsize=None)
def reference(name, mode, method, dtype=np.float64, mutation=None):
    """The specification on what the kernel reads (logits rounded to bf16 first in bf16 mode), in `dtype`.
    dict: obj, aux (mask_best, iou, box_args ...), dlogits [B, ch, cw, D]."""
    c = case(name)
    t = np.dtype(dtype).type
    obj, aux, dl = S.loss(H.inputs64(c['net'], mode).astype(t), c['labels'], c['anchors'], H.HP, c['C'], method, mutation)
    return dict(obj=obj, aux=aux, dlogits=dl)


def zero_box_net(c, logit=-120.0):
    """c's logits (float64 copy) with the size logits of every anchor of every object cell at `logit`: exp underflows, the boxes are 0 x 0."""
    net = c['net'].astype(np.float64).reshape(c['B'], c['ch'] * c['cw'], c['A'], 5 + c['C']).copy()
    net[c['labels'][0][..., 0] != 0, :, 3:5] = logit
    return net.reshape(c['net'].shape)


def box_channels(c, dlogits):
    """Channels 1..4 of every anchor: [B, ch, cw, A, 4]."""
    return np.asarray(dlogits).reshape(c['B'], c['ch'], c['cw'], c['A'], 5 + c['C'])[..., 1:5]


def other_channels(c, dlogits):
    """Channel 0 and channels 5.. of every anchor: [B, ch, cw, A, 1 + C]."""
    d = np.asarray(dlogits).reshape(c['B'], c['ch'], c['cw'], c['A'], 5 + c['C'])
    return np.concatenate([d[..., :1], d[..., 5:]], -1)


def kink_distance(name, mode):
    """Smallest distance (cells; cells^2 for the floors) of a responsible lane of the float64 reference from a kink: a tie of a predicted
    and a target edge, an axis in which the intersection is about to become empty or non-empty, the 1e-10 floors of U, E and c^2."""
    aux = reference(name, mode, 'ciou')['aux']
    sx, sy, w, h, X1, Y1, X2, Y2, At = [np.broadcast_to(a, aux['mask_best'].shape) for a in aux['box_args']]
    p = S._pieces(np, sx, sy, w, h, X1, Y1, X2, Y2, At)
    resp = aux['mask_best'] != 0
    d = [np.abs(p['x1'] - X1), np.abs(p['x2'] - X2), np.abs(p['y1'] - Y1), np.abs(p['y2'] - Y2), np.abs(p['rx']), np.abs(p['ry']),
         p['uraw'] - S.FLOOR, p['ew'] * p['eh'] - S.FLOOR, p['ew'] ** 2 + p['eh'] ** 2 - S.FLOOR]
    return float(min(x[resp].min() for x in d))


def smallest_r2(name, mode):
    """Smallest w^2 + h^2 of a responsible lane: the derivative of v floors it at 1e-30, which only underflow may reach (`tie_all`'s 1e-5-cell
    boxes sit at 1e-10, so this floor is measured by its own scale, not by KINK)."""
    aux = reference(name, mode, 'ciou')['aux']
    w, h = [np.broadcast_to(a, aux['mask_best'].shape)[aux['mask_best'] != 0] for a in aux['box_args'][2:4]]
    return float((w * w + h * h).min())
