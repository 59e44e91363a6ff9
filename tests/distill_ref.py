"""SPECIFICATION of objectness-scaled distillation between two YOLOv2 heads (csrc/distill.hip; Mehta & Ozturk, "Object
detection at 200 frames per second", ECCV-W 2018) -- test infrastructure, NumPy, float64 for references.

Logits are [B, cells, A, 5 + C] in the project's channel order iou, x, y, w, h, classes.  n = B cells A, s a lane of the student, t of the
teacher, sg the sigmoid.  The teacher is a constant: no derivative flows through it.

    m          = sg(t0) with scale_by_objectness, else 1
    objectness = 1/n sum (sg(s0) - sg(t0))^2
    coords     = 1/n sum m [(sg(s1) - sg(t1))^2 + (sg(s2) - sg(t2))^2 + (s3 - t3)^2 + (s4 - t4)^2]
                 (w and h as logits: the anchors are shared, so this is the log ratio of the two boxes' sides and no exp can overflow)
    prob       = 1/n sum m sum_k (p_k - q_k)^2                   class_term mse, p = softmax(s[5:] / T), q = softmax(t[5:] / T)
               = 1/n sum m T^2 sum_k q_k (log q_k - log p_k)     class_term kl, from the log-softmax
    total      = weight (w_objectness objectness + w_coords coords + w_prob prob)
    g          = d total / d s, in closed form (`gradient`)

`terms` is written against an array namespace `xp` (numpy or torch) so that tests/test_distill_cpu.py can differentiate this very forward with
torch float64 autograd and compare `gradient`, written by hand, against it.  `mutation` switches in the mistakes the mutation proofs of that
test need; None is the specification.

The kernel ADDS g into the gradient the loss launch stored: dl = store(f32(dl) + g).  In bf16 that rounds twice, once in the loss's store and
once here; `accumulate` is that second store."""
import numpy as np

from oracle import yolo2_ref as R

CLASS_TERMS = ('mse', 'kl')
MUTATIONS = ('no_scale', 'no_inv_T', 'sign_w')
DEFAULTS = dict(weight=1.0, objectness=1.0, coords=1.0, prob=1.0, class_term='mse', temperature=1.0, scale_by_objectness=True)


def options(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def _sigmoid(xp, x):
    return 1 / (1 + xp.exp(-x))


def _log_softmax(xp, z):
    mx = z.max(-1, keepdims=True) if xp is np else z.max(-1, keepdim=True).values
    d = z - mx
    return d - xp.log(xp.exp(d).sum(-1, keepdims=True) if xp is np else xp.exp(d).sum(-1, keepdim=True))


def terms(xp, s, t, opt, mutation=None):
    """The three unweighted objectives (objectness, coords, prob) of s, t [B, cells, A, 5 + C], with xp = numpy or torch."""
    n = s.shape[0] * s.shape[1] * s.shape[2]
    T = opt['temperature']
    to = _sigmoid(xp, t[..., 0])
    m = to if (opt['scale_by_objectness'] and mutation != 'no_scale') else to * 0 + 1
    objectness = ((_sigmoid(xp, s[..., 0]) - to) ** 2).sum() / n
    box = ((_sigmoid(xp, s[..., 1:3]) - _sigmoid(xp, t[..., 1:3])) ** 2).sum(-1) + ((s[..., 3:5] - t[..., 3:5]) ** 2).sum(-1)
    coords = (m * box).sum() / n
    lp, lq = _log_softmax(xp, s[..., 5:] / T), _log_softmax(xp, t[..., 5:] / T)
    p, q = xp.exp(lp), xp.exp(lq)
    if opt['class_term'] == 'mse':
        cls = ((p - q) ** 2).sum(-1)
    else:
        assert opt['class_term'] == 'kl', opt['class_term']
        cls = T * T * (q * (lq - lp)).sum(-1)
    prob = (m * cls).sum() / n
    return objectness, coords, prob


def total(opt, objectness, coords, prob):
    return opt['weight'] * (opt['objectness'] * objectness + opt['coords'] * coords + opt['prob'] * prob)


def gradient(s, t, opt, mutation=None):
    """d total / d s, written by hand, in float64 [B, cells, A, 5 + C]."""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    n = s.shape[0] * s.shape[1] * s.shape[2]
    T, W = opt['temperature'], opt['weight']
    sg_s, sg_t = _sigmoid(np, s[..., :3]), _sigmoid(np, t[..., :3])
    m = sg_t[..., 0] if (opt['scale_by_objectness'] and mutation != 'no_scale') else np.ones_like(sg_t[..., 0])
    e = np.exp(-np.abs(s[..., :3]))
    dsg = e / (1 + e) ** 2                       # sg'(z), accurate where the sigmoid saturates
    g = np.zeros_like(s)
    g[..., 0] = W * opt['objectness'] * 2 * (sg_s[..., 0] - sg_t[..., 0]) * dsg[..., 0] / n
    wc = W * opt['coords'] * m[..., None] / n
    g[..., 1:3] = wc * 2 * (sg_s[..., 1:3] - sg_t[..., 1:3]) * dsg[..., 1:3]
    g[..., 3:5] = wc * 2 * (s[..., 3:5] - t[..., 3:5])
    if mutation == 'sign_w':
        g[..., 3] = -g[..., 3]
    p, q = np.exp(_log_softmax(np, s[..., 5:] / T)), np.exp(_log_softmax(np, t[..., 5:] / T))
    wp = W * opt['prob'] * m[..., None] / n
    inv_T = 1.0 if mutation == 'no_inv_T' else 1.0 / T
    if opt['class_term'] == 'mse':
        d = 2 * (p - q)
        g[..., 5:] = wp * inv_T * p * (d - (d * p).sum(-1, keepdims=True))
    else:
        g[..., 5:] = wp * (T * T) * inv_T * (p - q)
    return g


def loss(s, t, mutation=None, **kw):
    """s, t [B, cells, A, 5 + C] -> (dict objectness, coords, prob, distill (the weighted sum), g float64)."""
    opt = options(**kw)
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    o, c, p = (float(v) for v in terms(np, s, t, opt, mutation))
    return {'objectness': o, 'coords': c, 'prob': p, 'distill': total(opt, o, c, p)}, gradient(s, t, opt, mutation)


def accumulate(d0, g, mode):
    """What a correct kernel leaves in dlogits that held d0 (already in its dtype): f32(d0) + g rounded to f32, then to bf16 in bf16 mode."""
    out = (np.asarray(d0, np.float32).astype(np.float64) + np.asarray(g, np.float64)).astype(np.float32)
    return (R.bf16_round(out) if mode == 'bf16' else out).astype(np.float64)


def accumulate_ratio(out, d0, g_ref, mode):
    """Worst |out - (d0 + g_ref)| / bound of an accumulated gradient.  bf16: 2^-8 |d0 + g_ref| + 1e-4 |g_ref| + 1e-5 max|g_ref|, half a bf16 ulp of the
    stored sum plus the f32 tolerance of the arithmetic before it; f32: the last two terms plus half an f32 ulp (2^-24) of the sum."""
    out, d0, g_ref = (np.asarray(a, np.float64) for a in (out, d0, g_ref))
    want = d0 + g_ref
    ulp = 2.0 ** -8 if mode == 'bf16' else 2.0 ** -24
    bound = ulp * np.abs(want) + 1e-4 * np.abs(g_ref) + 1e-5 * np.abs(g_ref).max()
    return float((np.abs(out - want) / (bound + 1e-300)).max())
