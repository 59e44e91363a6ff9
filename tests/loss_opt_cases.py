"""Cases, option matrix, float64 references and bounds for the loss options (tests/loss_opt_ref.py is the specification; csrc/loss_opts.h and
csrc/head.hip the kernel).  tests/test_loss_opt_cpu.py checks the cases themselves and proves that the bounds catch wrong losses;
tests/test_loss_opt_gpu.py launches the kernel on them.

Cases: the thirteen geometries of head_cases.V2_SPECS in the modes each lists, plus

    g1x1       B = 40, 1x1, A = 5 (8 lanes a cell: 32 images per 256-lane workgroup); every third image has no object
    g2x3       B = 9, 2x3, A = 3 (24 lanes an image: a workgroup straddles ten image boundaries); every fourth image has no object
    dense19    B = 2, 19x19, A = 5: every cell of image 0 an object (361 staged boxes), image 1 has none (the empty list)
    dense32    B = 1, 32x32, A = 5, bf16: every cell an object, 1024 boxes -- more than the kernel stages, so it reads the label rows instead
    g32        B = 1, 32x32, A = 5, C = 20, bf16, 40 objects: the largest multi-scale grid
    placed     B = 2, 7x10: in every object cell anchor 0 predicts the target at 0.95 of its sides (IoU 0.9, responsible), anchor 1 at 0.837 (IoU 0.7,
               below the best: own-cell ignoring); anchor 2 of the EMPTY cell to the left predicts 0.9 of the target's sides 0.15 cells off its
               centre, IoU about 0.8 (cross-cell ignoring)
    multihot   B = 2, 5x6, A = 3, C = 5: two objects of different classes share a cell in each image (a label row with two bits)
    onehot_sat B = 2, 5x6, A = 3, C = 4: in the object cells the target class's logit is +16 or -16 against 0: its probability is within 1e-6 of 1
               or of 0 on every anchor

The planted anchors of `placed` are planted in g1x1, g2x3 and dense19 too (anchors 0 and 1 of every object cell), so that every IGNORE case
ignores lanes of object cells at both thresholds; `placed` and g2x3 also have the planted neighbour in an empty cell (a 1x1 grid has no second
cell, dense19 has no empty cell in the image that has objects: they cannot ignore a lane of an empty cell).

Bounds: head_cases.objective_ratio, grad_ratio; 1.0 is the bound."""
import functools

import numpy as np

import head_cases as H
import loss_opt_ref as S
from oracle import yolo2_ref as R

THRESHOLDS = (0.3, 0.6)
# the option matrix: each option alone; all together with box_loss ciou (both thresholds, gamma 2 and 1)
CONFIGS = {
    'ign3': dict(ignore_thresh=0.3),
    'ign6': dict(ignore_thresh=0.6),
    'rescore': dict(rescore=True),
    'ce': dict(class_loss='ce'),
    'ce_s': dict(class_loss='ce', label_smoothing=0.1),
    'focal0': dict(class_loss='focal', focal_gamma=0.0),
    'focal0_s': dict(class_loss='focal', focal_gamma=0.0, label_smoothing=0.1),
    'focal1': dict(class_loss='focal', focal_gamma=1.0),
    'focal1_s': dict(class_loss='focal', focal_gamma=1.0, label_smoothing=0.1),
    'focal2': dict(class_loss='focal', focal_gamma=2.0),
    'focal2_s': dict(class_loss='focal', focal_gamma=2.0, label_smoothing=0.1),
    'focal15_s': dict(class_loss='focal', focal_gamma=1.5, label_smoothing=0.1),      # an exponent the kernel takes through powf
    'all6': dict(box_loss='ciou', ignore_thresh=0.6, rescore=True, class_loss='focal', focal_gamma=2.0, label_smoothing=0.1),
    'all3': dict(box_loss='ciou', ignore_thresh=0.3, rescore=True, class_loss='ce', label_smoothing=0.1),
}
NEW_SPECS = {   # name -> (B, ch, cw, A, C, seed, modes)
    'g1x1':       (40, 1, 1, 5, 4, 51, H.MODES),
    'g2x3':       (9, 2, 3, 3, 4, 52, H.MODES),
    'dense19':    (2, 19, 19, 5, 3, 53, H.MODES),
    'dense32':    (1, 32, 32, 5, 2, 54, ('bf16',)),
    'g32':        (1, 32, 32, 5, 20, 55, ('bf16',)),
    'placed':     (2, 7, 10, 5, 4, 56, H.MODES),
    'multihot':   (2, 5, 6, 3, 5, 57, H.MODES),
    'onehot_sat': (2, 5, 6, 3, 4, 58, H.MODES),
}
CASES = list(H.V2_SPECS) + list(NEW_SPECS)
IGNORE_CASES = ('g1x1', 'g2x3', 'dense19', 'placed')       # cases built so that ignoring is certain (the docstring says where)
IGNORE_EMPTY_CELL = ('g2x3', 'placed')                     # ... and certain in an empty cell too
# tie_all's gradients sit below 1e-7 on saturated sigmoids, where s (1 - s) in float32 alone costs more than the bound (box_loss_cases says the same)
GRADIENT_CONDITION_EXEMPT = ('tie_all',)


def modes(name):
    return (H.V2_SPECS.get(name) or NEW_SPECS[name])[-1]


ALL = [(n, m, k) for n in CASES for m in modes(n) for k in CONFIGS]


def _labels(objs, B, C, cw, ch):
    """objs[b] = list of (row, col, ox, oy, w, h, cls), centre offset inside the cell and size in cell units."""
    outs = []
    for b in range(B):
        o = objs[b]
        cx = np.array([(c + ox) / cw for r, c, ox, oy, w, h, k in o], np.float64)
        cy = np.array([(r + oy) / ch for r, c, ox, oy, w, h, k in o], np.float64)
        w = np.array([x[4] / cw for x in o], np.float64)
        h = np.array([x[5] / ch for x in o], np.float64)
        coord = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32) if o else np.zeros((0, 4), np.float32)
        outs.append(R.transform_labels(np.array([x[6] for x in o], np.int64), coord, C, cw, ch, dtype=np.float64))
    return H._stack_labels(outs)


def _plant(net, anchors, b, cell, a, off, size):
    net[b, cell, a, 1:3] = H._logit(np.asarray(off, np.float64))
    net[b, cell, a, 3:5] = np.log(np.asarray(size, np.float64) / anchors[a].astype(np.float64))


def _plant_object_cell(net, anchors, b, cell, ox, oy, w, h):
    _plant(net, anchors, b, cell, 0, (ox, oy), (0.95 * w, 0.95 * h))          # IoU 0.9025: responsible
    _plant(net, anchors, b, cell, 1, (ox, oy), (0.837 * w, 0.837 * h))        # IoU 0.70, below the best


def _clear_of_thresholds(net, c, rng, frozen):
    """The ignore rule is an exact comparison M > t, so a lane whose M nearly equals a tested threshold could be decided differently by expf on
    the device and np.exp here with both being right.  With thousands of lanes no seed keeps all of them away from two thresholds, so the seed
    is replaced lane by lane: the box logits (channels 1..4) of every lane whose float64 M lies within 2 MARGIN (relative) of a threshold, in
    any dtype of the case, are redrawn until none does -- never a ``frozen`` lane [B, cells, A], one that carries a construction (the object
    cells of the tie cases, the planted anchors); tests/test_loss_opt_cpu.py asserts the result with head_cases.MARGIN itself.  Returns net itself if nothing was redrawn."""
    B, cells, A, C = c['B'], c['ch'] * c['cw'], c['A'], c['C']
    labels = H.labels64(c['labels'])
    allowed = ~frozen
    out = net
    for _ in range(50):
        near = np.zeros((B, cells, A), bool)
        for mode in c['modes']:
            M = S.max_gt_iou(R.model_decode(H.inputs64(out, mode), C, c['anchors'].astype(np.float64), training=True), labels)
            for t in THRESHOLDS:
                near |= np.abs(M - t) <= 2 * H.MARGIN * t
        if not near.any():
            return out
        assert allowed[near].all(), (c['name'], 'a constructed lane sits on a threshold')
        lanes = out.reshape(B, cells, A, 5 + C).copy()
        lanes[near, 1:5] = (rng.randn(int(near.sum()), 4) * 0.7).astype(np.float32)
        out = lanes.reshape(net.shape)
    raise AssertionError((c['name'], 'no draw keeps every lane off the thresholds'))


@functools.lru_cache(maxsize=None)
def case(name):
    """head_cases.v2_case's dict for a reused or a new case; callers must not write to it."""
    if name in H.V2_SPECS:
        c = H.v2_case(name)
        frozen = np.broadcast_to((c['labels'][0][..., 0] != 0)[..., None] & (H.V2_SPECS[name][6] not in ('randn', 'big')), (c['B'], c['ch'] * c['cw'], c['A']))
        net = _clear_of_thresholds(c['net'], c, np.random.RandomState(900 + H.V2_SPECS[name][7]), frozen)
        return c if net is c['net'] else dict(c, net=net)
    B, ch, cw, A, C, seed, case_modes = NEW_SPECS[name]
    rng = np.random.RandomState(seed)
    d, cells = 5 + C, ch * cw
    anchors = H.VOC_ANCHORS[:A].copy()
    net = rng.randn(B, cells, A, d) * 0.7
    objs = [[] for _ in range(B)]
    if name in ('g1x1', 'g2x3'):
        for b in range(B):
            if b % (3 if name == 'g1x1' else 4) == 0:
                continue
            cell = 0 if name == 'g1x1' else [1, 2, 4, 5][rng.randint(0, 4)]   # g2x3: never column 0, the cell to the left exists and is empty
            r, c = divmod(cell, cw)
            ox, oy = (0.1, rng.uniform(0.3, 0.7)) if name == 'g2x3' else tuple(rng.uniform(0.3, 0.7, 2))
            w, h = rng.uniform(0.5, 0.9, 2) * (1.0 if name == 'g1x1' else 2.0)
            objs[b].append((r, c, ox, oy, w, h, rng.randint(0, C)))
    elif name in ('dense19', 'dense32'):
        for cell in range(cells):
            r, c = divmod(cell, cw)
            objs[0].append((r, c, rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8), rng.uniform(0.5, 3.0), rng.uniform(0.5, 3.0), rng.randint(0, C)))
    elif name == 'g32':
        for cell in rng.choice(cells, 40, replace=False):
            r, c = divmod(int(cell), cw)
            objs[0].append((r, c, rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8), rng.uniform(1.0, 12.0), rng.uniform(1.0, 12.0), rng.randint(0, C)))
    elif name == 'placed':
        spots = [[(1, 2), (3, 5), (5, 8), (4, 2)], [(2, 3), (0, 6), (5, 5), (3, 8)]]
        for b in range(B):
            for r, c in spots[b]:
                objs[b].append((r, c, 0.1, rng.uniform(0.3, 0.7), rng.uniform(2.0, 3.0), rng.uniform(2.0, 3.0), rng.randint(0, C)))
    elif name == 'multihot':
        for b in range(B):
            for cell in rng.choice(cells, 4, replace=False):
                r, c = divmod(int(cell), cw)
                objs[b].append((r, c, rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8), rng.uniform(0.8, 3.0), rng.uniform(0.8, 3.0), rng.randint(0, C)))
            r, c, _, _, _, _, k = objs[b][0]                                   # a second object of another class in the first one's cell (it takes the box)
            objs[b].append((r, c, rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8), rng.uniform(0.8, 3.0), rng.uniform(0.8, 3.0), (k + 1 + rng.randint(0, C - 1)) % C))
    elif name == 'onehot_sat':
        for b in range(B):
            for j, cell in enumerate(rng.choice(cells, 5, replace=False)):
                r, c = divmod(int(cell), cw)
                k = rng.randint(0, C)
                objs[b].append((r, c, rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8), rng.uniform(0.8, 3.0), rng.uniform(0.8, 3.0), k))
                net[b, cell, :, 5:] = 0.0
                net[b, cell, :, 5 + k] = 16.0 if j % 2 == 0 else -16.0         # p = 1 - 3.4e-7, or 3.8e-8
    labels = _labels(objs, B, C, cw, ch)
    frozen = np.zeros((B, cells, A), bool)
    if name in IGNORE_CASES:
        for b in range(B):
            for r, c, ox, oy, w, h, _ in objs[b]:
                if name == 'dense19' and (r * cw + c) % 7:
                    continue                                                   # one object cell in seven carries the planted anchors
                _plant_object_cell(net, anchors, b, r * cw + c, ox, oy, w, h)
                frozen[b, r * cw + c, :2] = True
                if name in IGNORE_EMPTY_CELL:
                    frozen[b, r * cw + c - 1, 2] = True
                    _plant(net, anchors, b, r * cw + c - 1, 2, (0.95, oy), (0.9 * w, 0.9 * h))       # the empty cell to the left, 0.15 cells off the centre
    resp = labels[0][..., 0].astype(np.int64)
    D = A * d
    net = net.reshape(B, ch, cw, D).astype(np.float32)
    c = dict(name=name, B=B, ch=ch, cw=cw, A=A, C=C, D=D, ld=H.pad8(D), net=net, anchors=anchors, labels=labels, modes=case_modes, resp=resp, objs=objs)
    c['net'] = _clear_of_thresholds(net, c, rng, frozen)
    c['net'].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def decoded(name, mode, dtype=np.float64):
    c = case(name)
    t = np.dtype(dtype).type
    net = H.inputs64(c['net'], mode).astype(t)
    return R.model_decode(net, c['C'], c['anchors'].astype(t), training=True), tuple(l.astype(t) for l in c['labels'])


@functools.lru_cache(maxsize=None)
def max_gt_iou(name, mode, dtype=np.float64):
    """M of every lane, once per case and dtype (shared by every configuration with a threshold; read only)."""
    M = S.max_gt_iou(*decoded(name, mode, dtype))
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def reference(name, mode, config, dtype=np.float64, mutation=None):
    """The specification on what the kernel reads, in `dtype`, for a configuration of CONFIGS (or 'off').  dict: obj, aux, dlogits [B, ch, cw, D]."""
    c = case(name)
    t = np.dtype(dtype).type
    kw = CONFIGS[config] if config != 'off' else {}
    M = max_gt_iou(name, mode, dtype) if kw.get('ignore_thresh', 0) > 0 and mutation is None else None
    obj, aux, dl = S.loss(H.inputs64(c['net'], mode).astype(t), c['labels'], c['anchors'], H.HP, c['C'], mutation=mutation, M=M, **kw)
    return dict(obj=obj, aux=aux, dlogits=dl)


def lanes(c, dlogits):
    """[B, ch, cw, D] -> [B, cells, A, 5 + C]."""
    return np.asarray(dlogits).reshape(c['B'], c['ch'] * c['cw'], c['A'], 5 + c['C'])


def concerned(config):
    """(objective indices, channel selector) an option set concerns: channel 0 for ignore / rescore, 5.. for a class mode, 1..4 for a box loss."""
    kw = CONFIGS[config]
    objs, chans = [], []
    if kw.get('ignore_thresh', 0) > 0:
        objs.append(1), chans.append('obj')
    if kw.get('rescore'):
        objs.append(0), chans.append('obj')
    if kw.get('class_loss', 'mse') != 'mse':
        objs.append(3), chans.append('cls')
    if kw.get('box_loss', 'mse') != 'mse':
        objs.append(2), chans.append('box')
    return sorted(set(objs)), sorted(set(chans))


def channels(c, dlogits, which):
    d = lanes(c, dlogits)
    return {'obj': d[..., :1], 'box': d[..., 1:5], 'cls': d[..., 5:]}[which]
