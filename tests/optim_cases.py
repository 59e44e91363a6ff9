"""Inputs, float64 references and error bounds for csrc/optim.hip: the seven optimizers (csrc/adam.h for Adam's arithmetic), the two per-tensor
clips, scale, zero_ranges and bn_fold.  NumPy and oracle/yolo2_ref.py only: tests/test_optim_cases_cpu.py checks the cases and the bounds on
a machine without a GPU (the f32 oracle fits every bound; ten planted faults each leave one), tests/test_optim_gpu.py launches the kernels.

Reference.  `step(kind, hp, state, g, gs, ty)` restates the oracle's *_step functions over the number type `ty` (test_optim_cases_cpu.py
holds it to R.*_step bit for bit in f32 and f64); the reference of a kernel launch is step(..., np.float64) on exactly the f32 values the
kernel reads: g * gs rounded to f32 first, as every kernel forms it, hyper-parameters as the f32 numbers the ABI passes (1 - beta, 1 - decay
and 1 - rho as the f32 differences the entry points and kernels form), Adam's alpha computed in double precision from the unrounded
hyper-parameters as yolo_tf_amd/optim.py does and then rounded to f32.

Every step is compared on its own arithmetic (`run_chain`): the state the device holds BEFORE step t is read back, and the reference of step
t is the float64 oracle applied to that state and g_t.  Over T = 12 steps the state ranges evolve (v shrinking and growing, accumulators
growing, |linear| crossing l1) and no bound on the amplification of earlier errors is needed.

Bounds (derived, not fitted; per element and per output array).  u = 2^-24:
    slots     |got - ref|     <= c u A + c TINY
    weights   |got_w - ref_w| <= u |ref_w| + c u A_update + c TINY
A is the output's own expression evaluated on the absolute values of its terms (a running-error bound: `acc * mom + g` that cancels is
still held to |acc| mom + |g|, and a small update is held to its own size, not to max |w|).  c is the number of f32 roundings on the longest
path of the expression, plus 2; the count is written next to each formula in `bounds`.  optim.hip is built with floating-point contraction
allowed, which can only remove roundings (a fused g * gs differs from the rounded one by at most u |g gs|, which every A contains);
adam_one has contraction off.  TINY = 2^-126, the smallest normal f32: an operation whose exact result lies below it may lose all of it (a
square that underflows), whether the hardware rounds gradually or flushes.  Ftrl's new weight is not `w - update` but the quotient x / y, so
it is bounded like a slot.  Ftrl with a general power is the one exception to "derived": the error of device powf is not derivable here, so
each powf value is allowed the project's existing 2e-5 relative (tests/test_kernels_gpu.py::test_optimizers_vs_oracle), propagated through the
same expressions (`extra`); the sqrt form gets the derived bound alone.

Ftrl's decision |linear| > l1.  At step 1 the elements i % 16 in {1, 2, 3} have w = 0 and g = 0, so the new linear is the old one without
any rounding, and the old one is planted: exactly +-l1, the f32 below it and the f32 above it.  Every other
element of a case with l1 > 0 must lie at least twice the bound of `linear` away from l1: `settle` multiplies a gradient that would land
closer by 1.5 (and raises one too small to matter to 0.37 l1 / gs) until it does not (it sees the state the step starts from, so this holds for the device's own chain too), and `check` reports
the smallest distance.  With l1 = 0 the decision is linear != 0: an f32 evaluation gives an exact 0 where every term is 0 (g = 0, linear = 0:
the elements i % 16 == 5) and otherwise only by a coincidence of its roundings.  The elements i % 32 == 5 also start with accum = 0: with l1 =
l2 = 0 the quotient there is 0 / 0, which `>` never selects and `>=` would.

Clip: float64 R.clip_by_norm per segment.  A segment whose float64 norm is at most `clip` must come back bit for bit; a clipped one within
5 u |ref| (the norm rounded to f32, the quotient, the product: 3 roundings + 2; the float64 sum's own error is 2^-29 of that).  zero_ranges,
scale: bit equality.  bn_fold: s = gamma / sqrt(var + eps) has 3 roundings, Wf = W s 4 (c = 6, A = |W s|), bias = beta - mean s 5 (c = 7,
A = |beta| + |mean s|)."""
import functools
import math

import numpy as np

from oracle import yolo2_ref as R

f32 = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -126
T = 12
GSCALES = (1.0, 1.0 / 3, 1.0 / 8)
SIZES = (1, 3, 4, 5, 255, 1023, 1024, 1025, 10007)
STRIDED = 2 * 8192 * 256 * 4 + 5          # adam_kernel and the OPT_LOOP kernels run their grid-stride loop twice from 8192 * 256 (* 4) elements on
POW_RTOL = 2e-5                           # device powf, not derivable (see the module docstring)

# name -> (kernel, learning rate, hyper-parameters as yolo_tf_amd/optim.py holds them: Python doubles)
CONFIGS = {
    'adam': ('adam', 1e-3, {'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}),
    'momentum': ('momentum', 0.01, {'momentum': 0.9}),
    'gd': ('gd', 0.01, {}),
    'rmsprop': ('rmsprop', 0.01, {'decay': 0.9, 'momentum': 0.5, 'epsilon': 1e-10}),
    'adagrad': ('adagrad', 0.01, {}),
    'adadelta': ('adadelta', 1.0, {'rho': 0.95, 'epsilon': 1e-8}),
    'ftrl_sqrt': ('ftrl', 0.05, {'learning_rate_power': -0.5, 'l1_regularization_strength': 0.0, 'l2_regularization_strength': 0.0}),
    'ftrl_sqrt_l1_l2': ('ftrl', 0.05, {'learning_rate_power': -0.5, 'l1_regularization_strength': 0.05, 'l2_regularization_strength': 0.01}),
    'ftrl_pow_l1': ('ftrl', 0.05, {'learning_rate_power': -0.7, 'l1_regularization_strength': 0.02, 'l2_regularization_strength': 0.0}),
}
SLOTS = {'adam': ('m', 'v'), 'momentum': ('acc',), 'gd': (), 'rmsprop': ('ms', 'mom'), 'adagrad': ('acc',), 'adadelta': ('acc', 'accu'),
         'ftrl': ('accum', 'linear')}
MUTATIONS = ('adam_eps_in_sqrt', 'adam_t_off_by_one', 'gscale_after_square', 'adadelta_updated_accu', 'rmsprop_eps_outside_sqrt',
             'momentum_lr_on_g', 'ftrl_ge', 'clip_f32_sum', 'clip_nan_ignored', 'zero_ranges_a_down')


def F(x):
    """The f32 number a float argument of the ABI holds, as a Python double."""
    return float(f32(x))


def one_minus(x):
    """1.0f - x as the entry points (Adam, RMSProp) and adadelta_kernel form it: one f32 subtraction (exact for x in [0.5, 1])."""
    return float(f32(1) - f32(x))


def alpha_of(hp, lr, t, mut=None):
    """yolo_tf_amd/optim.py Optimizer.apply: double precision, unrounded hyper-parameters."""
    if mut == 'adam_t_off_by_one':
        t = t + 1
    return lr * math.sqrt(1.0 - hp['beta2'] ** t) / (1.0 - hp['beta1'] ** t)


def scaled(g, gs):
    """g * gs in f32, the first thing every kernel computes."""
    return np.asarray(g, f32) * f32(gs)


# ------------------------------------------------------------------------------------------------------------------
# the update rules over a number type (oracle/yolo2_ref.py *_step, with switches for the mistakes a kernel could make)
# ------------------------------------------------------------------------------------------------------------------

def step(kind, hp, state, g, gs, ty, lr=None, alpha=None, mut=None):
    """state = (w, slot, ...) arrays -> the new state, every operation in `ty` (np.float32: the f32 oracle; np.float64: the reference).
    g f32, gs the gradient scale; lr for all but Adam, which takes alpha."""
    w, s = np.asarray(state[0], ty), [np.asarray(x, ty) for x in state[1:]]
    gi = scaled(g, gs).astype(ty)
    sq = (ty(F(gs)) * (np.asarray(g, ty) * np.asarray(g, ty))) if mut == 'gscale_after_square' else gi * gi
    c = lambda k: ty(F(hp[k]))
    with np.errstate(all='ignore'):
        if kind == 'adam':
            m, v = s
            m = m + (gi - m) * ty(one_minus(hp['beta1']))
            v = v + (sq - v) * ty(one_minus(hp['beta2']))
            den = np.sqrt(v + c('epsilon')) if mut == 'adam_eps_in_sqrt' else np.sqrt(v) + c('epsilon')
            return w - (m * ty(F(alpha))) / den, m, v
        lr = ty(F(lr))
        if kind == 'momentum':
            if mut == 'momentum_lr_on_g':
                acc = s[0] * c('momentum') + lr * gi
                return w - acc, acc
            acc = s[0] * c('momentum') + gi
            return w - lr * acc, acc
        if kind == 'gd':
            return (w - lr * gi,)
        if kind == 'rmsprop':
            ms, mom = s
            ms = ms + (sq - ms) * ty(one_minus(hp['decay']))
            den = (np.sqrt(ms) + c('epsilon')) if mut == 'rmsprop_eps_outside_sqrt' else np.sqrt(ms + c('epsilon'))
            mom = mom * c('momentum') + lr * gi / den
            return w - mom, ms, mom
        if kind == 'adagrad':
            acc = s[0] + sq
            return w - lr * gi / np.sqrt(acc), acc
        if kind == 'adadelta':
            acc, accu = s
            rho, omr = c('rho'), ty(one_minus(hp['rho']))
            acc = acc * rho + sq * omr
            upd = np.sqrt(accu + c('epsilon')) / np.sqrt(acc + c('epsilon')) * gi
            new_accu = accu * rho + upd * upd * omr
            if mut == 'adadelta_updated_accu':        # the slot is stored first and the update reads it back
                upd = np.sqrt(new_accu + c('epsilon')) / np.sqrt(acc + c('epsilon')) * gi
            return w - lr * upd, acc, new_accu
        if kind == 'ftrl':
            accum, linear = s
            p, l1, l2 = F(hp['learning_rate_power']), c('l1_regularization_strength'), c('l2_regularization_strength')
            na = accum + sq
            if p == -0.5:
                pa, pna = np.sqrt(accum), np.sqrt(na)
            else:
                pa, pna = np.power(accum, ty(-p)), np.power(na, ty(-p))
            linear = linear + (gi - (pna - pa) / lr * w)
            x = l1 * np.sign(linear) - linear
            y = pna / lr + ty(2) * l2
            on = (np.abs(linear) >= l1) if mut == 'ftrl_ge' else (np.abs(linear) > l1)
            return np.where(on, x / y, ty(0)).astype(ty), na, linear
    raise KeyError(kind)


def oracle_step(kind, hp, state, gi, lr, t):
    """The same step by oracle/yolo2_ref.py itself (gi: the scaled gradient in the dtype of the state): what `step` restates."""
    w, s = state[0], state[1:]
    if kind == 'adam':
        return R.adam_step(w, gi, s[0], s[1], lr, t, hp['beta1'], hp['beta2'], hp['epsilon'])
    if kind == 'momentum':
        return R.momentum_step(w, gi, s[0], lr, hp['momentum'])
    if kind == 'gd':
        return (R.gd_step(w, gi, lr),)
    if kind == 'rmsprop':
        return R.rmsprop_step(w, gi, s[0], s[1], lr, hp['decay'], hp['momentum'], hp['epsilon'])
    if kind == 'adagrad':
        return R.adagrad_step(w, gi, s[0], lr)
    if kind == 'adadelta':
        return R.adadelta_step(w, gi, s[0], s[1], lr, hp['rho'], hp['epsilon'])
    return R.ftrl_step(w, gi, s[0], s[1], lr, hp['learning_rate_power'], hp['l1_regularization_strength'], hp['l2_regularization_strength'])


# ------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------

def bounds(kind, hp, state, g, gs, lr=None, alpha=None):
    """name -> (c, A, extra) for 'w' and every slot, from the float64 reference of the step that starts at `state`; extra: an absolute
    allowance that is not a rounding count (Ftrl's powf only).  For Ftrl also 'decision': |(|linear| - l1)| over the bound of linear, inf
    where linear is computed without rounding (g = 0: new_accum = accum and linear stays; w = 0 and linear = 0: it is g * gs itself)."""
    w, s = np.asarray(state[0], np.float64), [np.asarray(x, np.float64) for x in state[1:]]
    gi = scaled(g, gs).astype(np.float64)
    ag, sq = np.abs(gi), gi * gi
    h = lambda k: F(hp[k])
    with np.errstate(all='ignore'):
        if kind == 'adam':
            m, v = s
            o1, o2, al, eps = one_minus(hp['beta1']), one_minus(hp['beta2']), F(alpha), h('epsilon')
            Am = np.abs(m) + (ag + np.abs(m)) * o1                   # m + (g - m) omb1: subtract, multiply, add = 3
            Av = np.abs(v) + (sq + np.abs(v)) * o2                   # v + (g g - v) omb2: square, subtract, multiply, add = 4
            v1 = v + (sq - v) * o2
            Au = Am * al / (np.sqrt(v1) + eps)                       # (m alpha) / (sqrt(v) + eps): v (4), sqrt, add, divide = 7
            return {'m': (3 + 2, Am, 0), 'v': (4 + 2, Av, 0), 'w': (7 + 2, Au, 0)}
        lr = F(lr)
        if kind == 'momentum':
            mo = h('momentum')
            Aa = np.abs(s[0]) * mo + ag                              # acc mom + g: multiply, add = 2
            return {'acc': (2 + 2, Aa, 0), 'w': (3 + 2, lr * Aa, 0)}  # lr acc: one more = 3
        if kind == 'gd':
            return {'w': (1 + 2, lr * ag, 0)}                        # lr g: 1
        if kind == 'rmsprop':
            ms, mom = s
            omd, mo, eps = one_minus(hp['decay']), h('momentum'), h('epsilon')
            As = np.abs(ms) + (sq + np.abs(ms)) * omd                # ms + (g g - ms) omd: square, subtract, multiply, add = 4
            s1 = ms + (sq - ms) * omd
            Amo = np.abs(mom) * mo + lr * ag / np.sqrt(s1 + eps)     # mom momentum + lr g / sqrt(ms + eps): ms (4), add, sqrt, divide, add = 8
            return {'ms': (4 + 2, As, 0), 'mom': (8 + 2, Amo, 0), 'w': (8 + 2, Amo, 0)}
        if kind == 'adagrad':
            a = s[0] + sq                                            # acc + g g: square, add = 2
            return {'acc': (2 + 2, np.abs(s[0]) + sq, 0), 'w': (4 + 2, lr * ag / np.sqrt(a), 0)}       # lr g / sqrt(acc): acc (2), sqrt, divide = 4
        if kind == 'adadelta':
            acc, accu = s
            rho, omr, eps = h('rho'), one_minus(hp['rho']), h('epsilon')
            Aa = np.abs(acc) * rho + sq * omr                        # acc rho + g g (1 - rho): square, multiply, add = 3
            a1 = acc * rho + sq * omr
            upd = np.sqrt(accu + eps) / np.sqrt(a1 + eps) * ag       # sqrt(accu + eps) / sqrt(acc + eps) g: acc (3), add, sqrt, divide, multiply = 7
            Au = np.abs(accu) * rho + upd * upd * omr                # accu rho + upd upd (1 - rho): upd (7), square, multiply, add = 10
            return {'acc': (3 + 2, Aa, 0), 'accu': (10 + 2, Au, 0), 'w': (8 + 2, lr * upd, 0)}         # lr upd: 8
        if kind == 'ftrl':
            accum, linear = s
            p, l1, l2 = h('learning_rate_power'), h('l1_regularization_strength'), h('l2_regularization_strength')
            na = accum + sq                                          # accum + g g: square, add = 2
            if p == -0.5:
                pa, pna, e = np.sqrt(accum), np.sqrt(na), 0.0        # sqrt(na): 3
            else:
                pa, pna, e = np.power(accum, -p), np.power(na, -p), POW_RTOL
            aw = np.abs(w)
            Al = np.abs(linear) + ag + (pna + pa) / lr * aw          # linear + (g - (pna - pa) / lr w): pna (3), subtract, divide, multiply, subtract, add = 8
            el = e * (pna + pa) / lr * aw                            # the two powf values, each off by e relative, through the same expression
            li = linear + (gi - (pna - pa) / lr * w)
            y = pna / lr + 2 * l2
            Aw = (l1 + Al) / y                                       # (l1 sign - linear) / (pna / lr + 2 l2): linear (8), subtract, divide = 10
            on = np.abs(li) > l1
            ew = np.where(on, el / y + e * (pna / lr) / y * np.abs((l1 * np.sign(li) - li) / y), 0.0)
            exact = (gi == 0) | ((w == 0) & (linear == 0))       # pna - pa is 0 - 0 and linear stays / linear is g itself
            dist = np.abs(np.abs(li) - l1)
            decision = np.where(exact | (dist == 0), np.inf, dist / ((8 + 2) * U * Al + el + TINY))
            return {'accum': (2 + 2, np.abs(accum) + sq, 0), 'linear': (8 + 2, Al, el), 'w_quotient': (10 + 2, np.where(on, Aw, 0.0), ew),
                    'decision': decision}
    raise KeyError(kind)


def ratio(got, ref, bound):
    """|got - ref| / bound per element; 0 where the two are equal (an exact result that is exact), inf where either is not finite."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(all='ignore'):
        r = np.where(got == ref, 0.0, np.abs(got - ref) / bound)
    return np.where(np.isfinite(r), r, np.inf)


def check(kind, hp, state, g, gs, new_state, lr=None, alpha=None):
    """The state `new_state` that a step (device or f32 oracle) produced from `state` against the float64 reference.
    -> {name: worst |err| / bound} over 'w' and the slots; for Ftrl also 'zero_pattern' (0.0 if w == 0 exactly where the reference is, else
    inf) and 'decision_distance' (the smallest distance of |linear| from l1 in bounds, over the elements not exactly on it)."""
    ref = step(kind, hp, state, g, gs, np.float64, lr=lr, alpha=alpha)
    b = bounds(kind, hp, state, g, gs, lr=lr, alpha=alpha)
    out = {}
    for name, r, got in zip(('w',) + SLOTS[kind], ref, new_state):
        if name == 'w' and kind != 'ftrl':
            c, A, extra = b['w']
            bound = U * np.abs(r) + c * U * A + c * TINY + extra
        else:
            c, A, extra = b['w_quotient' if name == 'w' else name]
            bound = c * U * A + c * TINY + extra
        out[name] = float(ratio(got, r, bound).max())
    if kind == 'ftrl':
        out['zero_pattern'] = 0.0 if np.array_equal(np.asarray(new_state[0]) == 0, ref[0] == 0) else np.inf
        if F(hp['l1_regularization_strength']) > 0:
            out['decision_distance'] = float(b['decision'].min())
    return out


# ------------------------------------------------------------------------------------------------------------------
# optimizer cases
# ------------------------------------------------------------------------------------------------------------------
ZERO_AT, UNDERFLOW_AT, NEAR_EPS_AT = 5, 9, 13      # i % 16: g exactly 0 / g ~ 1e-25 (the square underflows) / g ~ 3e-7 (Adam: sqrt(v) ~ eps), at every step
PLANT_AT = (1, 2, 3)                               # i % 16: Ftrl, step 1: |linear| exactly l1, just below, just above


def _seed(name, n, gs, t=0):
    return (sorted(CONFIGS).index(name) * 100003 + n * 131 + int(round(1 / gs)) * 17 + t) % (2 ** 31)


def init_state(name, n, gs):
    """The f32 state a chain starts from: (w, slots...).  Not the Optimizer's start values (tests/test_optim_gpu.py reads those back on their
    own): slots that already hold something, so that step 1 exercises every term."""
    kind, _, hp = CONFIGS[name]
    rng = np.random.RandomState(_seed(name, n, gs))
    i = np.arange(n)
    w = rng.randn(n).astype(f32)
    if kind == 'adam':
        return w, np.zeros(n, f32), np.zeros(n, f32)
    if kind == 'momentum':
        return w, (0.1 * rng.randn(n)).astype(f32)
    if kind == 'gd':
        return (w,)
    if kind == 'rmsprop':                                   # ms from 1e-14 (eps = 1e-10 decides the root) to 1, and exactly 1 (its start value)
        ms = (10.0 ** rng.uniform(-14, 0, n)).astype(f32)
        ms[i % 7 == 0] = 1.0
        return w, ms, (0.01 * rng.randn(n)).astype(f32)
    if kind == 'adagrad':
        acc = (0.1 + 0.1 * rng.rand(n)).astype(f32)
        acc[i % 16 == ZERO_AT] = 0.1
        return w, acc
    if kind == 'adadelta':
        return w, np.zeros(n, f32), np.zeros(n, f32)
    accum = np.full(n, 0.1, f32)
    accum[i % 32 == ZERO_AT] = 0.0                          # with g = 0 at every step: new_accum^-p stays 0, the quotient is 0 / 0 when l2 = 0
    linear = np.zeros(n, f32)
    l1 = f32(hp['l1_regularization_strength'])
    if l1 > 0:                                              # w = 0 and g_1 = 0 there: the new linear is the planted one, without any rounding
        w[np.isin(i % 16, PLANT_AT)] = 0.0
        sign = np.where(rng.rand(n) < 0.5, -1, 1).astype(f32)
        for k, target in zip(PLANT_AT, (l1, np.nextafter(l1, f32(0)), np.nextafter(l1, f32(np.inf)))):
            linear[i % 16 == k] = (sign * target)[i % 16 == k]
    return w, accum, linear


def gradient(name, n, gs, t):
    """g_t f32 [n]: magnitudes log-uniform over 1e-10 .. 1e2 with random sign; the special elements of ZERO_AT, UNDERFLOW_AT, NEAR_EPS_AT; at
    t = 1 zero in the planted Ftrl elements."""
    kind, _, hp = CONFIGS[name]
    rng = np.random.RandomState(_seed(name, n, gs, t))
    i = np.arange(n)
    sign = np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    g = (sign * 10.0 ** rng.uniform(-10, 2, n)).astype(f32)
    g[i % 16 == UNDERFLOW_AT] = (sign * 1e-25 * (1 + rng.rand(n))).astype(f32)[i % 16 == UNDERFLOW_AT]
    g[i % 16 == NEAR_EPS_AT] = (sign * 3e-7 * (1 + rng.rand(n))).astype(f32)[i % 16 == NEAR_EPS_AT]
    g[i % 16 == ZERO_AT] = 0.0
    if kind == 'ftrl' and F(hp['l1_regularization_strength']) > 0 and t == 1:
        g[np.isin(i % 16, PLANT_AT)] = 0.0
    return g


def settle(name, state, g, gs, lr):
    """Ftrl with l1 > 0: the gradient with every element whose |linear| would land within twice linear's bound of l1 (and is not computed
    exactly) multiplied by 1.5 until it does not.  Other cases: g unchanged."""
    kind, _, hp = CONFIGS[name]
    if kind != 'ftrl' or F(hp['l1_regularization_strength']) == 0:
        return g
    g = g.copy()
    l1 = f32(hp['l1_regularization_strength'])
    for k in range(8):
        near = bounds(kind, hp, state, g, gs, lr=lr)['decision'] < 2
        if not near.any():
            return g
        # (a gradient too small to move a linear that sits next to l1 is raised to 0.37 l1 / gs from the third attempt on)
        mag = np.maximum(np.abs(g[near]) * f32(1.5), f32(0.37) * l1 / f32(gs) if k >= 2 else f32(0))
        g[near] = np.where(g[near] < 0, -mag, mag).astype(f32)
    raise AssertionError('%s: %d elements stay within the bound of l1' % (name, int(near.sum())))


def run_chain(name, n, gs, stepper, steps=T, mut=None):
    """`steps` steps of case (name, n, gs).  stepper(kind, hp, state, g, gs, lr, alpha) -> the new f32 state (a tuple of NumPy arrays), by the
    device or by the f32 oracle; it gets the state of the previous step back.  Every step is checked against the float64 reference of that
    step.  -> {name: worst ratio over all steps} ('decision_distance': the smallest)."""
    kind, lr, hp = CONFIGS[name]
    state = init_state(name, n, gs)
    worst = {}
    for t in range(1, steps + 1):
        g = settle(name, state, gradient(name, n, gs, t), gs, lr)
        alpha = alpha_of(hp, lr, t) if kind == 'adam' else None
        new = stepper(kind, hp, state, g, gs, lr, alpha_of(hp, lr, t, mut) if kind == 'adam' else None)
        new = tuple(np.asarray(x, f32) for x in new)
        for k, v in check(kind, hp, state, g, gs, new, lr=lr, alpha=alpha).items():
            worst[k] = min(worst.get(k, np.inf), v) if k == 'decision_distance' else max(worst.get(k, 0.0), v)
        state = new
    return worst


def oracle32_stepper(mut=None):
    def stepper(kind, hp, state, g, gs, lr, alpha):
        return step(kind, hp, state, g, gs, f32, lr=lr, alpha=alpha, mut=mut)
    return stepper


# ------------------------------------------------------------------------------------------------------------------
# clip_by_norm, clip_by_norm_fixed
# ------------------------------------------------------------------------------------------------------------------
CLIP = 5.0
CLIP_C = 3 + 2          # the norm rounded to f32, clip / norm, g * scale; + 2
# (length, content): every length of 0, 1, 63, 64, 65, 257, 64 * 256 + 7, 70001 and every content at least once
CLIP_TABLE = ((70001, 'big'), (0, 'empty'), (1, 'eq_clip'), (63, 'tiny'), (64, 'zeros'), (65, 'below'), (257, 'overflow'), (64 * 256 + 7, 'big'),
              (0, 'empty'), (1, 'big'), (63, 'overflow'), (65, 'eq_clip'), (64 * 256 + 7, 'below'), (257, 'zeros'), (70001, 'below'), (64, 'tiny'))
CLIP_NONFINITE = ((300, 'big'), (100, 'inf'), (65, 'below'), (70, 'nan'), (300, 'big'))
CLIP_CASES = {'nseg1': CLIP_TABLE[:1], 'full_table': CLIP_TABLE, 'non_finite': CLIP_NONFINITE}


def _segment(rng, n, content):
    x = rng.randn(n)
    norm = np.sqrt((x * x).sum()) if n else 1.0
    if content in ('zeros', 'empty'):
        x = np.zeros(n)
    elif content in ('below', 'inf'):            # norm = clip / 1000: comes back bit for bit
        x = x / norm * CLIP * 1e-3
    elif content == 'eq_clip':                   # one element equal to clip, the others 0: the norm IS clip
        x = np.zeros(n)
        x[n // 2] = CLIP if n % 2 else -CLIP
    elif content in ('big', 'nan'):              # norm = 1e4 clip
        x = x / norm * CLIP * 1e4
    elif content == 'overflow':                  # every square overflows f32; the float64 sum is ~ 1e40 n
        x = np.sign(x) * 1e20 * (1 + rng.rand(n))
    elif content == 'tiny':                      # every square underflows f32
        x = np.sign(x) * 1e-30 * (1 + rng.rand(n))
    x = x.astype(f32)
    if content == 'inf':
        x[n // 3] = np.inf
    if content == 'nan':
        x[n // 3] = np.nan
    return x


@functools.lru_cache(maxsize=None)
def clip_case(name):
    """dict: g f32 (read-only), seg_off int64 [nseg + 1], nseg, contents."""
    table = CLIP_CASES[name]
    rng = np.random.RandomState(len(table))
    g = np.concatenate([_segment(rng, n, c) for n, c in table])
    g.setflags(write=False)
    off = np.concatenate([[0], np.cumsum([n for n, _ in table])]).astype(np.int64)
    return dict(g=g, seg_off=off, nseg=len(table), contents=[c for _, c in table])


def clip_model32(g, seg_off, clip, mut=None):
    """seg_sumsq_kernel + seg_scale_kernel restated: float64 sum of squares, the norm and the scale in f32."""
    out = np.array(g, f32)
    for s in range(len(seg_off) - 1):
        x = out[seg_off[s]:seg_off[s + 1]]
        with np.errstate(all='ignore'):
            ss = np.float64((x * x).sum(dtype=f32)) if mut == 'clip_f32_sum' else (x.astype(np.float64) ** 2).sum()
            norm = f32(np.sqrt(ss))
            if np.isnan(norm) and mut != 'clip_nan_ignored':
                scale = norm
            else:
                scale = f32(clip) / np.fmax(norm, f32(clip))        # fmaxf: the other operand when one is NaN
            if scale != f32(1):
                x *= scale
    return out


def clip_check(got, g, seg_off, clip):
    """-> (worst |err| / (5 u |ref|) over the clipped finite elements, list of complaints).  Per segment against float64 R.clip_by_norm: a
    segment whose norm is at most clip bit for bit, NaN where and only where the reference has NaN."""
    worst, bad = 0.0, []
    got = np.asarray(got, f32)
    for s in range(len(seg_off) - 1):
        a, b = int(seg_off[s]), int(seg_off[s + 1])
        x, y = np.asarray(g[a:b], f32), got[a:b]
        with np.errstate(all='ignore'):
            x64 = x.astype(np.float64)
            ref = R.clip_by_norm(x64, F(clip))
            norm = np.sqrt((x64 ** 2).sum())
        if norm <= F(clip):
            if not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
                bad.append('segment %d [%d, %d): norm %g <= clip, but %d elements changed' % (s, a, b, norm, int((x.view(np.uint32) != y.view(np.uint32)).sum())))
            continue
        if not np.array_equal(np.isnan(ref), np.isnan(y)):
            bad.append('segment %d [%d, %d): %d NaN, the reference has %d' % (s, a, b, int(np.isnan(y).sum()), int(np.isnan(ref).sum())))
            continue
        ok = ~np.isnan(ref)
        r = float(ratio(y[ok], ref[ok], CLIP_C * U * np.abs(ref[ok])).max()) if ok.any() else 0.0
        worst = max(worst, r)
        if r > 1:
            bad.append('segment %d [%d, %d): worst |err| / (5 u |ref|) = %.3g' % (s, a, b, r))
    return worst, bad


# ------------------------------------------------------------------------------------------------------------------
# zero_ranges
# ------------------------------------------------------------------------------------------------------------------
SENTINEL = np.uint32(0xDEADBEEF)        # -6.26e18 as f32: not zero, not NaN


def _slots(k, width, length):
    """k ranges in disjoint slots of `width` elements: range j starts at j mod 4 within its slot and is length(j) long."""
    return [(j * width + j % 4, j * width + j % 4 + length(j)) for j in range(k)]


def zero_ranges_cases():
    """name -> (n, ranges)."""
    pairs = [(k * 32 + a, k * 32 + a + ln) for k, (a, ln) in enumerate((a, ln) for a in range(4) for ln in range(10))]
    return {
        'short_branch': (16, [(1, 3), (5, 7), (9, 10), (14, 15)]),                      # a4 > b4: no 16-byte body
        'every_a_mod_4_b_mod_4_lengths_0_to_9': (40 * 32 + 5, pairs),                 # 36 non-empty ranges: three launches
        'scalar_edges_long': (200003, [(1, 100003), (100006, 150001), (150003, 150004), (160000, 199999)]),
        'adjacent_and_to_the_end': (1031, [(3, 10), (10, 17), (17, 1031)]),
        'multi_launch_17_ranges': (17 * 40, _slots(17, 40, lambda j: 5 + j % 9)),
        'multi_launch_33_ranges': (33 * 40, _slots(33, 40, lambda j: 1 + j % 13)),
    }


ZERO_RANGES_STRIDED = (STRIDED, [(3, STRIDED - 2)])      # the 16-byte body loop strides


def zero_ranges_model(x, ranges, mut=None):
    """x uint32 -> a copy with every [a, b) zeroed."""
    out = np.array(x, np.uint32)
    for a, b in ranges:
        if b > a:
            out[(a & ~3) if mut == 'zero_ranges_a_down' else a:b] = 0
    return out


def zero_ranges_branches(ranges):
    """Which parts of zero_ranges_kernel a list of ranges reaches: (short branch, body, left edge, right edge, launches)."""
    short = body = left = right = False
    nonempty = 0
    for a, b in ranges:
        if b <= a:
            continue
        nonempty += 1          # (empty ranges are dropped per group of 16 ranges; the launches are counted below)
        a4, b4 = (a + 3) & ~3, b & ~3
        if a4 <= b4:
            body |= b4 > a4
            left |= a4 > a
            right |= b > b4
        else:
            short = True
    launches = sum(1 for i0 in range(0, len(ranges), 16) if any(b > a for a, b in ranges[i0:i0 + 16]))
    return short, body, left, right, launches


# ------------------------------------------------------------------------------------------------------------------
# scale, bn_fold
# ------------------------------------------------------------------------------------------------------------------
SCALE_FACTORS = (1.0 / 3, -1.0, 0.0, 1e-3)


def scale_input(n):
    return np.random.RandomState(n % 65521).randn(n).astype(f32)


BN_FOLD_SHAPES = ((1, 1), (27, 32), (9, 3), (1152, 125), (4608, 1024))
BN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def bn_fold_case(rows, C):
    """dict: W [rows, C], gamma, beta, mean, var f32 [C].  gamma negative in c % 5 == 4 and 0 in c % 5 == 2; var 0 in c % 7 == 3; mean = beta / s in
    c % 3 == 1, so that beta - mean s cancels."""
    rng = np.random.RandomState(rows * 1031 + C)
    c = np.arange(C)
    W = rng.randn(rows, C).astype(f32)
    gamma = rng.uniform(0.5, 1.5, C)
    gamma[c % 5 == 4] *= -1
    gamma[c % 5 == 2] = 0
    var = rng.uniform(0.01, 4.0, C)
    var[c % 7 == 3] = 0
    beta, mean = rng.randn(C), rng.randn(C)
    gamma, beta, var = gamma.astype(f32), beta.astype(f32), var.astype(f32)
    s = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + F(BN_EPS))
    cancel = (c % 3 == 1) & (s != 0)
    mean[cancel] = beta[cancel] / s[cancel]
    out = dict(W=W, gamma=gamma, beta=beta, mean=mean.astype(f32), var=var, cancel=cancel)
    for v in out.values():
        v.setflags(write=False)
    return out


def bn_fold_model(case, ty):
    s = case['gamma'].astype(ty) / np.sqrt(case['var'].astype(ty) + ty(F(BN_EPS)))
    return case['W'].astype(ty) * s, case['beta'].astype(ty) - case['mean'].astype(ty) * s


def bn_fold_check(Wf, bias, case):
    """-> (worst ratio of Wf, worst ratio of bias)."""
    rw, rb = bn_fold_model(case, np.float64)
    s = case['gamma'].astype(np.float64) / np.sqrt(case['var'].astype(np.float64) + F(BN_EPS))
    Ab = np.abs(case['beta'].astype(np.float64)) + np.abs(case['mean'].astype(np.float64) * s)
    return (float(ratio(np.asarray(Wf).reshape(rw.shape), rw, (4 + 2) * U * np.abs(rw) + TINY).max()),
            float(ratio(bias, rb, (5 + 2) * U * Ab + TINY).max()))
