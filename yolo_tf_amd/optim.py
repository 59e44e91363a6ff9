"""Optimizers and learning-rate schedule with the reference's configuration surface
(train.py:70-80 get_optimizer, :116-124 exponential_decay; config.ini [optimizer_*],
[exponential_decay]).  Each optimizer is ONE kernel launch over the flat parameter arena
(csrc/optim.hip; Adam fused with the filter re-layout: csrc/filter_prep.hip), with TF-1.0 Apply* update rules."""
import configparser
import math

import torch

from . import ops, options


LR_POLICIES = options.KEYS['lr_policy'].choices
LR_KEYS = ('lr_policy', 'lr_steps', 'lr_scales', 'lr_max_steps', 'lr_power', 'lr_min_ratio', 'burn_in', 'burn_in_power')


def learning_rate_fn(config, base_lr):
    """The learning rate of the update whose 0-based count (``global_step``) is ``step``, in Python floats.

    With none of the ``[mi355x]`` schedule keys (LR_KEYS) present: lr * decay_rate ** floor(step / decay_steps) when [exponential_decay] is present, else
    constant (reference train.py:116-124), the function as it was before the keys existed.  Otherwise:

    ``lr_policy`` = exponential | constant | steps | poly | cosine (absent: [exponential_decay] when present, else constant)
      steps   base * prod(lr_scales[i] for lr_steps[i] <= step)                                  (Darknet's policy = steps, steps, scales)
      poly    base * (1 - s / max) ** lr_power                                                    (lr_power defaults to 4)
      cosine  base * (lr_min_ratio + (1 - lr_min_ratio) * (1 + cos(pi * s / max)) / 2)            (lr_min_ratio defaults to 0)
      with s = min(step, max) and max = ``lr_max_steps`` (train.py writes its -s there when the key is absent).
    ``burn_in`` = N, ``burn_in_power`` (default 4, Darknet's): the policy's value times min(1, (step + 1) / N) ** power -- step + 1, so that the first
    update is not a zero update.  ValueError names the key for an unknown policy, lr_steps and lr_scales of different lengths, poly or cosine without a
    max, and negative values.  Pure host logic."""
    if not any(options.has(config, key) for key in LR_KEYS):
        return _reference_learning_rate_fn(config, base_lr)
    raw = options.read(config, 'lr_policy')
    policy = raw.strip().lower() if raw is not None else None
    if policy is not None and policy not in LR_POLICIES:
        raise ValueError('[mi355x] lr_policy = %r: one of %s' % (raw, ', '.join(LR_POLICIES)))
    for key in ('lr_steps', 'lr_scales'):
        if options.has(config, key) and policy != 'steps':
            raise ValueError('[mi355x] %s belongs to lr_policy = steps, not %s' % (key, policy or 'the default policy'))

    def numbers(key, one=True):          # none negative: the key's list, or with ``one`` the single number it must hold; absent: its default
        if not options.has(config, key):
            return options.KEYS[key].default
        values = options.read(config, key, how='list', invalid='not a list of numbers')
        if any(v < 0 for v in values):
            raise options.refusal(config, key, 'negative')
        if one and len(values) != 1:
            raise options.refusal(config, key, 'one number')
        return values[0] if one else values
    if policy is None:
        fn = _reference_learning_rate_fn(config, base_lr)
    elif policy == 'exponential':
        if not config.has_section('exponential_decay'):
            raise ValueError('[mi355x] lr_policy = exponential: the config has no [exponential_decay] section')
        fn = _reference_learning_rate_fn(config, base_lr)
    elif policy == 'constant':
        fn = lambda step: base_lr
    elif policy == 'steps':
        at, scales = list(numbers('lr_steps', one=False)), list(numbers('lr_scales', one=False))
        if len(at) != len(scales):
            raise ValueError('[mi355x] lr_steps has %d entries and lr_scales %d: one scale per step' % (len(at), len(scales)))
        if sorted(at) != at:
            raise options.refusal(config, 'lr_steps', 'not ascending')

        def fn(step):
            lr = base_lr
            for a, s in zip(at, scales):
                if a <= step:
                    lr *= s
            return lr
    else:
        top = numbers('lr_max_steps')
        if top <= 0:
            raise ValueError('[mi355x] lr_policy = %s needs a positive lr_max_steps (or train.py -s)' % policy)
        if policy == 'poly':
            power = numbers('lr_power')
            fn = lambda step: base_lr * (1.0 - min(step, top) / top) ** power
        else:
            floor = numbers('lr_min_ratio')
            if floor > 1.0:
                raise ValueError('[mi355x] lr_min_ratio = %r: lies in [0, 1]' % floor)
            fn = lambda step: base_lr * (floor + (1.0 - floor) * 0.5 * (1.0 + math.cos(math.pi * min(step, top) / top)))
    burn = numbers('burn_in')
    burn_power = numbers('burn_in_power')
    if burn <= 0:
        return fn
    return lambda step: fn(step) * min(1.0, (step + 1) / burn) ** burn_power


def _reference_learning_rate_fn(config, base_lr):
    """lr * decay_rate ** floor(step / decay_steps) when [exponential_decay] is present, else constant
    (reference train.py:116-124)."""
    try:
        steps = config.getint('exponential_decay', 'decay_steps')
        rate = config.getfloat('exponential_decay', 'decay_rate')
        staircase = config.getboolean('exponential_decay', 'staircase')
    except (configparser.NoSectionError, configparser.NoOptionError, AttributeError):
        return lambda step: base_lr

    def fn(step):
        p = step / steps
        if staircase:
            p = math.floor(p)
        return base_lr * rate ** p
    return fn


DEFAULTS = {
    'adam': {'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8},
    'adadelta': {'rho': 0.95, 'epsilon': 1e-8},
    'adagrad': {'initial_accumulator_value': 0.1},
    'momentum': {'momentum': 0.9},
    'rmsprop': {'decay': 0.9, 'momentum': 0.0, 'epsilon': 1e-10},
    'ftrl': {'learning_rate_power': -0.5, 'initial_accumulator_value': 0.1, 'l1_regularization_strength': 0.0, 'l2_regularization_strength': 0.0},
    'gd': {},
}


class Optimizer(object):
    def __init__(self, name, config, n, device):
        if name not in DEFAULTS:
            raise KeyError('optimizer %r is not available on this path (adam, adadelta, adagrad, momentum, rmsprop, ftrl, gd)' % name)
        self.name = name
        self.hp = dict(DEFAULTS[name])
        section = 'optimizer_' + name
        if config is not None and config.has_section(section):
            for key in self.hp:
                if config.has_option(section, key):
                    self.hp[key] = config.getfloat(section, key)
        self.n = n
        from .engine import staggered          # (arena placement: see engine.staggered)
        z = lambda fill=0.0: staggered(n, torch.float32, device, fill)
        self.slots = {
            'adam': lambda: [z(), z()], 'adadelta': lambda: [z(), z()],
            'adagrad': lambda: [z(self.hp.get('initial_accumulator_value', 0.1))], 'momentum': lambda: [z()],
            'rmsprop': lambda: [z(1.0), z()],          # [TF-sem] RMSProp's `rms` slot starts at ones
            'ftrl': lambda: [z(self.hp['initial_accumulator_value']), z()],     # accum, linear
            'gd': lambda: [],
        }[name]()

    def apply_fused_with_filter_prep(self, engine, lr, t, gscale=1.0):
        """Adam over the whole arena and the operand layouts of the updated filters in one launch (engine.adam_update_and_prepare);
        bit-identical to ``apply`` followed by the engine's filter preparation."""
        assert self.name == 'adam'
        hp = self.hp
        alpha = lr * math.sqrt(1.0 - hp['beta2'] ** t) / (1.0 - hp['beta1'] ** t)
        engine.adam_update_and_prepare(self.slots[0], self.slots[1], alpha, hp['beta1'], hp['beta2'], hp['epsilon'], gscale)

    def apply(self, params, grads, lr, t, gscale=1.0, lo=0, hi=None):
        """t = 1-based update count (Adam bias correction).  [lo, hi) restricts the update to a slice of the flat arenas
        (data parallel: one call per all-reduce bucket as the buckets arrive)."""
        hp = self.hp
        hi = self.n if hi is None else hi
        n = hi - lo
        if lo != 0 or hi != self.n:
            params, grads = params[lo:hi], grads[lo:hi]
        s = [slot[lo:hi] for slot in self.slots] if (lo != 0 or hi != self.n) else self.slots
        if self.name == 'adam':
            alpha = lr * math.sqrt(1.0 - hp['beta2'] ** t) / (1.0 - hp['beta1'] ** t)
            ops.adam(params, grads, s[0], s[1], n, alpha, hp['beta1'], hp['beta2'], hp['epsilon'], gscale)
        elif self.name == 'momentum':
            ops.momentum(params, grads, s[0], n, lr, hp['momentum'], gscale)
        elif self.name == 'gd':
            ops.sgd(params, grads, n, lr, gscale)
        elif self.name == 'rmsprop':
            ops.rmsprop(params, grads, s[0], s[1], n, lr, hp['decay'], hp['momentum'], hp['epsilon'], gscale)
        elif self.name == 'adagrad':
            ops.adagrad(params, grads, s[0], n, lr, gscale)
        elif self.name == 'ftrl':
            ops.ftrl(params, grads, s[0], s[1], n, lr, hp['learning_rate_power'], hp['l1_regularization_strength'], hp['l2_regularization_strength'], gscale)
        elif self.name == 'adadelta':
            ops.adadelta(params, grads, s[0], s[1], n, lr, hp['rho'], hp['epsilon'], gscale)
