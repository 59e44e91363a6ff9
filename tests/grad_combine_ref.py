"""NumPy specification of yolo2_grad_combine (include/yolo2_hip.h): gradient accumulation over micro-batches, their mean and weight
decay, in f32 with the kernel's operation order -- every operation rounded once.  Test infrastructure only: the product never imports it."""
import numpy as np

STORE, ADD, FINAL = 0, 1, 2


def mask(n, ranges):
    """Boolean [n]: the elements inside the sorted, disjoint half-open ``ranges``."""
    m = np.zeros(n, bool)
    for b, e in ranges:
        m[b:e] = True
    return m


def combine(g, acc, w, mode, scale=1.0, decay=0.0, shrink=1.0, ranges=()):
    """-> (g, acc, w) after the launch, as new arrays (None stays None).  FINAL: s = g; with acc s = acc + s; s = s * scale; inside a range and decay != 0
    s = s + decay * w (the product rounded, then the sum); g = s; inside a range and shrink != 1 w = w * shrink."""
    f32 = np.float32
    g = np.array(g, f32, copy=True)
    acc = None if acc is None else np.array(acc, f32, copy=True)
    w = None if w is None else np.array(w, f32, copy=True)
    with np.errstate(all='ignore'):          # NaN and inf propagate as IEEE says
        if mode == STORE:
            return g, g.copy(), w
        if mode == ADD:
            return g, np.add(acc, g, dtype=f32), w
        assert mode == FINAL
        s = g
        if acc is not None:
            s = np.add(acc, s, dtype=f32)
        s = np.multiply(s, f32(scale), dtype=f32)
        m = mask(len(g), ranges)
        if m.any() and f32(decay) != 0:
            t = np.multiply(f32(decay), w[m], dtype=f32)
            s[m] = np.add(s[m], t, dtype=f32)
        if m.any() and f32(shrink) != 1:
            w[m] = np.multiply(w[m], f32(shrink), dtype=f32)
        return s, acc, w


def accumulate(grads, w, decay=0.0, shrink=1.0, ranges=()):
    """What a TrainSession with accum_steps = len(grads) hands its optimizer: STORE, ADD ..., then FINAL with scale = f32(1 / K) over the
    micro-gradients ``grads`` (K = 1: FINAL without an accumulator).  -> (gradient, w)."""
    K = len(grads)
    acc = None
    for k, g in enumerate(grads[:-1]):
        _, acc, _ = combine(g, acc, None, STORE if k == 0 else ADD)
    g, _, w = combine(grads[-1], acc, w, FINAL, np.float32(1.0 / K), decay, shrink, ranges)
    return g, w


def weight_ranges(param_offsets):
    """The decayed ranges of an arena laid out as ``param_offsets`` {name: (offset, size)}: the variables named .../weights, sorted by offset."""
    return sorted((o, o + n) for name, (o, n) in param_offsets.items() if name.rsplit('/', 1)[-1] == 'weights')
