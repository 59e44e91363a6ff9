"""Inputs, float64 references and error bounds for the head kernels (csrc/head.hip: YOLOv2 loss + decode; csrc/yolo1.hip: v1 loss +
decode).  NumPy and oracle/yolo2_ref.py only: tests/test_head_cases_cpu.py checks the cases themselves on a machine without a GPU,
tests/test_head_gpu.py launches the kernels on them.

The reference is the oracle in float64 on exactly the values a kernel reads: the logits (rounded to bf16 first in bf16 mode), f32
labels and f32 anchors, all widened unchanged.  Every case and every reference is built once and cached; callers must not write to
them.

Responsibility is an exact float comparison (`iou == max_A iou`), so an input whose two best IoUs nearly coincide could be resolved
differently by expf on the device and np.exp here with both being right.  `margins` measures that: in every object cell the top IoUs
are either exactly equal (the deliberate ties) or the best exceeds the next distinct value by more than MARGIN relative.  The seeds
below were chosen so that this holds for every case in both dtypes; a seed that violated it would be replaced, never the margin."""
import functools

import numpy as np

from oracle import yolo2_ref as R

F32_RTOL = 1e-4               # the project's f32 tolerance (tests/test_kernels_gpu.py)
F32_FLOOR = 0.1 * F32_RTOL    # assert_close's floor, relative to max|ref|
BF16_HALF_ULP = 2.0 ** -8     # round-to-nearest bf16 (8 significand bits): |x - bf16(x)| <= 2^-9 * 2^e <= 2^-8 |x|
MARGIN = 1e-3
HP = {'iou_best': 5., 'iou_normal': 1., 'coords': 2., 'prob': .5}      # distinct, so that a swapped weight shows
HPARAM = [HP[k] for k in R.OBJECTIVE_KEYS]
VOC_ANCHORS = np.array([[1.08, 1.19], [3.42, 4.41], [6.63, 11.38], [9.42, 5.11], [16.62, 10.52]], np.float32)
MODES = ('f32', 'bf16')


def pad8(c):
    return (c + 7) // 8 * 8


def inputs64(x, mode):
    """What the kernel reads, widened: bf16 mode rounds the logits to bf16 (round-to-nearest-even) first."""
    return (R.bf16_round(x) if mode == 'bf16' else np.asarray(x, np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------
# bounds (shared by the GPU tests and by the mutation proofs of the CPU test)
# ------------------------------------------------------------------------------------------------------------------

def f32_ratio(got, ref):
    """Worst |err| / bound of test_kernels_gpu.assert_close(got, ref, F32_RTOL): per element 1e-4 |ref| + 1e-5 max|ref|."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max() + 1e-30
    return float((np.abs(got - ref) / (F32_RTOL * np.abs(ref) + F32_FLOOR * scale)).max())


def bf16_ratio(got, ref):
    """Worst |err| / bound for a bf16-stored gradient: per element (2^-8 + 1e-4) |ref| + 1e-5 max|ref| -- half a bf16 ulp of
    round-to-nearest, plus the f32 tolerance of the arithmetic before the store, plus the f32 floor.  Derived, not measured;
    truncation (error up to 2^-7 |ref|) does not fit."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max() + 1e-30
    return float((np.abs(got - ref) / ((BF16_HALF_ULP + F32_RTOL) * np.abs(ref) + F32_FLOOR * scale)).max())


def grad_ratio(got, ref, mode):
    return bf16_ratio(got, ref) if mode == 'bf16' else f32_ratio(got, ref)


def objective_ratio(got, ref):
    """|err| / (F32_RTOL |ref|) of one objective; the same bound in both dtypes (f32 arithmetic on rounded inputs)."""
    return abs(float(got) - float(ref)) / (F32_RTOL * abs(float(ref)) + 1e-300)


def bf16_truncate(x):
    """The wrong store: the upper 16 bits of the f32 value, no rounding."""
    a = np.ascontiguousarray(x, np.float32)
    return (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).reshape(a.shape)


def stored(grad64, mode, store=R.bf16_round):
    """A correct kernel's output for the exact gradient grad64: f32, or f32 rounded to bf16 by `store`."""
    g = np.asarray(grad64, np.float64).astype(np.float32)
    return (store(g) if mode == 'bf16' else g).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------
# labels
# ------------------------------------------------------------------------------------------------------------------

def _stack_labels(per_image):
    """Per-image transform_labels tuples (float64) -> 6 batch arrays in f32, the dtype they have on the device."""
    return tuple(np.stack([o[i] for o in per_image]).astype(np.float32) for i in range(6))


def labels64(labels):
    return tuple(l.astype(np.float64) for l in labels)


def _random_labels(rng, B, classes, cw, ch, kmin=4, kmax=7):
    """Boxes as in tests/test_kernels_gpu.py `_labels` (centres in 0.05..0.95, sides 0.05..0.6 of the image, clipped), f32 coordinates,
    at least kmin of them per image so that two images give eight object cells."""
    outs = []
    for _ in range(B):
        k = rng.randint(kmin, kmax)
        cen = rng.uniform(0.05, 0.95, (k, 2))
        wh = rng.uniform(0.05, 0.6, (k, 2))
        coord = np.clip(np.concatenate([cen - wh / 2, cen + wh / 2], 1), 0, 1).astype(np.float32)
        outs.append(R.transform_labels(rng.randint(0, classes, k), coord, classes, cw, ch, dtype=np.float64))
    return _stack_labels(outs)


def _placed_labels(rng, B, classes, cw, ch, k, offset, size_cells):
    """k objects per image in k distinct cells.  offset(rng) -> (ox, oy) of the centre inside its cell, size_cells(rng) -> (w, h)
    in cell units.  Returns (labels, cells [B, k] flat indices, offsets [B, k, 2], sizes [B, k, 2])."""
    outs, cells, offs, sizes = [], [], [], []
    for _ in range(B):
        idx = rng.choice(ch * cw, k, replace=False)
        o = np.array([offset(rng) for _ in range(k)], np.float64)
        s = np.array([size_cells(rng) for _ in range(k)], np.float64)
        cx, cy = (idx % cw + o[:, 0]) / cw, (idx // cw + o[:, 1]) / ch
        w, h = s[:, 0] / cw, s[:, 1] / ch
        coord = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32)
        lab = R.transform_labels(rng.randint(0, classes, k), coord, classes, cw, ch, dtype=np.float64)
        assert np.array_equal(np.flatnonzero(lab[0][:, 0]), np.sort(idx))       # every box landed in the cell it was placed in
        outs.append(lab)
        cells.append(idx), offs.append(o), sizes.append(s)
    return _stack_labels(outs), np.array(cells), np.array(offs), np.array(sizes)


# ------------------------------------------------------------------------------------------------------------------
# YOLOv2 cases: name -> (B, cell_h, cell_w, A, C, ld or None for pad8, recipe, seed, modes)
# ------------------------------------------------------------------------------------------------------------------
V2_SPECS = {
    'sq13_ld136':  (2, 13, 13, 5, 20, 136, 'randn', 11, MODES),       # 1: the existing f32 test's geometry, 8 more padding channels
    'rect9x14':    (3, 9, 14, 5, 80, None, 'randn', 12, MODES),       # 2: cell_h < cell_w, 80 classes
    'rect19x11':   (2, 19, 11, 5, 20, None, 'big', 13, MODES),        # 3: cell_h > cell_w, big logits
    'a1':          (2, 7, 10, 1, 4, None, 'randn', 14, MODES),        # 4: LPC 1, the butterfly loop is skipped
    'a2':          (2, 7, 10, 2, 4, None, 'randn', 15, MODES),        #    LPC 2
    'a3':          (2, 7, 10, 3, 4, None, 'randn', 16, MODES),        #    LPC 4, one idle lane
    'a8':          (2, 7, 10, 8, 4, None, 'randn', 17, MODES),        #    LPC 8, no idle lane, D*A = 72 = pad8: no padding channel
    'a8_ld80':     (2, 7, 10, 8, 4, 80, 'randn', 17, MODES),          #    the same values with 8 padding channels
    'a9':          (2, 7, 10, 9, 4, None, 'randn', 18, MODES),        #    LPC 16, seven idle lanes
    'a33':         (2, 5, 6, 33, 3, None, 'randn', 19, MODES),        #    LPC 64: 31 idle lanes, a cell per wave
    'b8_19x19':    (8, 19, 19, 5, 20, None, 'randn', 20, ('bf16',)),  # 5: 91 workgroups: the finalisation's 64-lane loop wraps, last workgroup partly idle
    'tie_all':     (2, 7, 10, 5, 6, None, 'tie_all', 21, MODES),      # 6a: every IoU of an object cell is exactly 0 -> five responsible anchors
    'tie_pair':    (2, 7, 10, 5, 6, None, 'tie_pair', 22, MODES),     # 6b: two identical anchors with identical logits
}
V2_DECODE_CASES = ['sq13_ld136', 'rect9x14', 'rect19x11', 'a1', 'a2', 'a3', 'a8', 'a8_ld80', 'a9', 'a33']      # cases 1 to 4


def _anchors(A, seed):
    if A <= 5:
        return VOC_ANCHORS[:A].copy()
    return np.random.RandomState(1000 + seed).uniform(0.5, 12, (A, 2)).astype(np.float32)


def _logit(p):
    return np.log(p / (1 - p))


@functools.lru_cache(maxsize=None)
def v2_case(name):
    """dict: B, ch, cw, A, C, D (real channels), ld, net f32 [B, ch, cw, D], anchors f32 [A, 2], labels (6 f32 arrays [B, cells, ...]),
    modes, resp int [B, cells]: the number of responsible anchors the construction intends per cell (0 where there is no object)."""
    B, ch, cw, A, C, ld, recipe, seed, modes = V2_SPECS[name]
    rng = np.random.RandomState(seed)
    d, cells = 5 + C, ch * cw
    D = A * d
    anchors = _anchors(A, seed)
    if recipe == 'randn':
        net = rng.randn(B, cells, A, d) * 0.7
        labels = _random_labels(rng, B, C, cw, ch)
        resp = labels[0][..., 0].astype(np.int64)
    elif recipe == 'big':       # large but finite in f32: exp(4) * 16.62 cells wide at most, sigmoid saturating to within an ulp of 0 and 1
        net = np.concatenate([rng.randn(B, cells, A, 3) * 5, np.clip(rng.randn(B, cells, A, 2) * 3, -6, 4), rng.randn(B, cells, A, C) * 8], -1)
        labels = _random_labels(rng, B, C, cw, ch)
        resp = labels[0][..., 0].astype(np.int64)
    elif recipe == 'tie_all':
        # a 0.1-cell target in one corner of its cell, every predicted box 1e-4 cells wide in the opposite corner: no overlap, IoU exactly 0
        net = rng.randn(B, cells, A, d) * 0.7
        corner = lambda r: tuple(r.choice([0.12, 0.88], 2))
        labels, idx, offs, _ = _placed_labels(rng, B, C, cw, ch, 5, corner, lambda r: (0.1, 0.1))
        for b in range(B):
            for i, o in zip(idx[b], offs[b]):
                net[b, i, :, 1:3] = np.where(o < 0.5, 8.0, -8.0)
                net[b, i, :, 3:5] = -12.0
        resp = labels[0][..., 0].astype(np.int64) * A
    elif recipe == 'tie_pair':
        # anchors 1 and 3 are the same box and carry the same logits in the object cells.  Every box sits 0.1 cells off the target's centre.
        # Even object cells: the pair predicts 0.8 of the target's sides (IoU ~ 0.6), the rest 0.4 (IoU ~ 0.16).  Odd object cells: anchor 0
        # has the 0.8 box, the pair the 0.4 box, anchors 2 and 4 a 0.25 box (IoU ~ 0.06).
        anchors[3] = anchors[1]
        net = rng.randn(B, cells, A, d) * 0.7
        labels, idx, offs, sizes = _placed_labels(rng, B, C, cw, ch, 5, lambda r: tuple(r.uniform(0.25, 0.75, 2)), lambda r: tuple(r.uniform(1.5, 4.0, 2)))
        resp = np.zeros((B, cells), np.int64)
        for b in range(B):
            for j, (i, o, s) in enumerate(zip(idx[b], offs[b], sizes[b])):
                pair_wins = j % 2 == 0
                scale = np.array([0.8, 0.4, 0.25, 0.4, 0.25]) if not pair_wins else np.array([0.4, 0.8, 0.4, 0.8, 0.4])
                net[b, i, :, 1:3] = _logit(o + 0.1)
                net[b, i, :, 3:5] = np.log(s[None, :] * scale[:, None] / anchors.astype(np.float64))
                net[b, i, 3] = net[b, i, 1]
                resp[b, i] = 2 if pair_wins else 1
    else:
        raise KeyError(recipe)
    net = net.reshape(B, ch, cw, D).astype(np.float32)
    net.setflags(write=False)
    return dict(name=name, B=B, ch=ch, cw=cw, A=A, C=C, D=D, ld=ld or pad8(D), net=net, anchors=anchors, labels=labels, modes=modes, resp=resp)


@functools.lru_cache(maxsize=None)
def v2_reference(name, mode, dtype=np.float64):
    """Oracle on what the kernel reads.  dict: m (Model attributes, detection ones included), obj, aux, iou, dlogits [B, ch, cw, D]."""
    c = v2_case(name)
    t = np.dtype(dtype).type
    net = inputs64(c['net'], mode).astype(t)
    labels = tuple(l.astype(t) for l in c['labels'])
    m = R.model_decode(net, c['C'], c['anchors'].astype(t), training=False)
    obj, aux = R.objectives(m, labels)
    dl = R.loss_backward(m, labels, aux, HP, c['C'])
    return dict(m=m, obj=obj, aux=aux, iou=aux['iou'], dlogits=dl)


def margins(iou, mask):
    """Per object cell: (number of anchors at the maximum, relative gap from the maximum to the next distinct IoU; inf if there is none)."""
    out = []
    for b, cell in zip(*np.nonzero(mask.reshape(mask.shape[0], -1))):
        v = np.unique(iou[b, cell])
        top = v[-1]
        out.append((int((iou[b, cell] == top).sum()), float((top - v[-2]) / top) if len(v) > 1 else np.inf))
    return out


# ------------------------------------------------------------------------------------------------------------------
# The oracle's loss restated in one function, with switches for the mistakes a kernel could make.  mutation=None must equal
# R.objectives / R.loss_backward; each mutation must leave the bounds above on at least one case (tests/test_head_cases_cpu.py).
# ------------------------------------------------------------------------------------------------------------------
MUTATIONS = ('swap_cell_wh', 'class_mask', 'first_max', 'swap_iou_weights', 'anchor_mod5')      # plus the bf16 truncation, which is a store


def v2_restated(name, mode, mutation=None):
    """(objectives dict, dlogits [B, ch, cw, D]) in float64."""
    c = v2_case(name)
    B, ch, cw, A, C = c['B'], c['ch'], c['cw'], c['A'], c['C']
    z = inputs64(c['net'], mode).reshape(B, ch * cw, A, 5 + C)
    mask, tprob, tcoords, tmin, tmax, tareas = labels64(c['labels'])
    anchors = c['anchors'].astype(np.float64)
    if mutation == 'anchor_mod5':
        anchors = anchors[np.arange(A) % 5]
    sg = 1 / (1 + np.exp(-z[..., :3]))
    wh = np.exp(z[..., 3:5]) * anchors.reshape(1, 1, A, 2)
    grid = np.array([ch, cw] if mutation == 'swap_cell_wh' else [cw, ch], np.float64)
    sq = np.sqrt(wh / grid)
    e = np.exp(z[..., 5:] - z[..., 5:].max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    pmin, pmax = sg[..., 1:3] - wh / 2, sg[..., 1:3] + wh / 2
    iwh = np.maximum(np.minimum(pmax, tmax) - np.maximum(pmin, tmin), 0)
    inter = iwh[..., 0] * iwh[..., 1]
    iou = inter / np.maximum(tareas + wh[..., 0] * wh[..., 1] - inter, 1e-10)
    if mutation == 'first_max':
        best = (np.arange(A).reshape(1, 1, A) == iou.argmax(2)[..., None]).astype(np.float64)
    else:
        best = (iou == iou.max(2, keepdims=True)).astype(np.float64)
    mb = mask * best
    mc = (mask * np.ones_like(best) if mutation == 'class_mask' else mb)[..., None]
    w_best, w_normal = (HP['iou_normal'], HP['iou_best']) if mutation == 'swap_iou_weights' else (HP['iou_best'], HP['iou_normal'])
    cnt = float(mb.size)
    coords = np.concatenate([sg[..., 1:3], sq], -1)
    obj = {'iou_best': (mb * (sg[..., 0] - mb) ** 2).sum() / cnt, 'iou_normal': ((1 - mb) * (sg[..., 0] - mb) ** 2).sum() / cnt,
           'coords': (mb[..., None] * (coords - tcoords) ** 2).sum() / cnt, 'prob': (mc * (p - tprob) ** 2).sum() / cnt}
    dz = np.zeros_like(z)
    s = sg[..., 0]
    dz[..., 0] = 2 * (s - mb) * (w_best * mb + w_normal * (1 - mb)) / cnt * s * (1 - s)
    sxy = sg[..., 1:3]
    dz[..., 1:3] = 2 * mb[..., None] * (sxy - tcoords[..., :2]) * HP['coords'] / cnt * sxy * (1 - sxy)
    dz[..., 3:5] = 2 * mb[..., None] * (sq - tcoords[..., 2:4]) * HP['coords'] / cnt * sq / 2
    d = 2 * mc * (p - tprob) * HP['prob'] / cnt
    dz[..., 5:] = p * (d - (d * p).sum(-1, keepdims=True))
    return obj, dz.reshape(B, ch, cw, A * (5 + C))


# ------------------------------------------------------------------------------------------------------------------
# YOLO (v1) cases: name -> (B, cell_h, cell_w, boxes, C, padding beyond pad8(width), seed).  The network output is linear: [cells*C | cells*boxes*5].
# ------------------------------------------------------------------------------------------------------------------
V1_SPECS = {
    'v1_3x4_b2': (3, 3, 4, 2, 5, 0, 31),         # width 180 -> ld 184
    'v1_4x3_b3': (2, 4, 3, 3, 5, 8, 32),         # width 240 = pad8: a row of 8 padding values only because ld is 248; LPC 4, one idle lane
    'v1_5x5_b1': (2, 5, 5, 1, 4, 0, 33),         # LPC 1
}


@functools.lru_cache(maxsize=None)
def v1_case(name):
    """dict: B, ch, cw, boxes, C, width, ld, net f32 [B, width], labels, resp [B, cells], zero_cell and tie_cell (image, cell).  Object cells predict the target's centre within
    0.15 and its sides within 0.6..1.4, so the IoUs are positive and distinct.  In image 0 the first object cell has sqrt_w exactly 0 in
    every box (all IoUs 0: every box responsible, and the |x| gradient is taken at 0), the second has boxes 0 and 1 identical and
    matching the target, a third box (if there is one) 0.4 of its sides."""
    B, ch, cw, boxes, C, extra, seed = V1_SPECS[name]
    rng = np.random.RandomState(seed)
    cells = ch * cw
    width = cells * (C + boxes * 5)
    labels, idx, offs, sizes = _placed_labels(rng, B, C, cw, ch, 4, lambda r: tuple(r.uniform(0.25, 0.75, 2)), lambda r: tuple(r.uniform(0.1, 0.5, 2) * [cw, ch]))
    cls = rng.randn(B, cells, C) * 0.5
    box = rng.randn(B, cells, boxes, 5) * 0.5
    resp = labels[0][..., 0].astype(np.int64)
    zero_cell, tie_cell = (0, int(idx[0][0])), ((0, int(idx[0][1])) if boxes > 1 else None)
    for b in range(B):
        for j, (i, o, s) in enumerate(zip(idx[b], offs[b], sizes[b])):
            root = np.sqrt(s / [cw, ch])                                       # the target's sqrt(w01), sqrt(h01)
            box[b, i, :, 1:3] = o + rng.uniform(-0.15, 0.15, (boxes, 2))
            box[b, i, :, 3:5] = root * rng.uniform(0.6, 1.4, (boxes, 2)) * rng.choice([-1.0, 1.0], (boxes, 2))
            if b == 0 and j == 0:
                box[b, i, :, 3] = 0.0
                resp[b, i] = boxes
            if b == 0 and j == 1 and boxes > 1:
                box[b, i, :, 1:3] = o
                box[b, i, :, 3:5] = root * [1.0, -1.0]
                if boxes > 2:
                    box[b, i, 2:, 3:5] *= 0.4
                box[b, i, 1] = box[b, i, 0]
                resp[b, i] = 2
    net = np.concatenate([cls.reshape(B, -1), box.reshape(B, -1)], 1).astype(np.float32)
    net.setflags(write=False)
    return dict(name=name, B=B, ch=ch, cw=cw, boxes=boxes, C=C, width=width, ld=pad8(width) + extra, net=net, labels=labels, resp=resp,
                zero_cell=zero_cell, tie_cell=tie_cell)


def iou_of(m, labels):
    """model/yolo2/__init__.py:73-78 (the same lines in model/yolo/__init__.py) on a decoded model: IoU [B, cells, boxes]."""
    _, _, _, tmin, tmax, tareas = labels
    iwh = np.maximum(np.minimum(m['offset_xy_max'], tmax) - np.maximum(m['offset_xy_min'], tmin), 0)
    inter = iwh[..., 0] * iwh[..., 1]
    return inter / np.maximum(tareas + m['areas'] - inter, 1e-10)


@functools.lru_cache(maxsize=None)
def v1_reference(name, mode, dtype=np.float64):
    c = v1_case(name)
    t = np.dtype(dtype).type
    net = inputs64(c['net'], mode).astype(t)
    labels = tuple(l.astype(t) for l in c['labels'])
    m = R.yolo1_model_decode(net, c['C'], c['boxes'], c['ch'], c['cw'], training=False)
    obj, aux = R.yolo1_objectives(m, labels)
    dnet = R.yolo1_loss_backward(m, labels, aux, HP, c['C'], c['boxes'], c['width'])
    return dict(m=m, obj=obj, aux=aux, iou=iou_of(m, labels), dnet=dnet)
