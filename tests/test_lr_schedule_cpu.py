"""optim.learning_rate_fn with the [mi355x] schedule keys: known answers for every policy and for burn-in, the keys absent against
the function as it was on the shipped config.ini, and every error.  Pure host logic."""
import configparser
import math
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 1e-3


def cfg(text='', exponential=False):
    c = configparser.ConfigParser()
    c.read_string(('[exponential_decay]\ndecay_steps = 100\ndecay_rate = 0.5\nstaircase = true\n' if exponential else '') + ('[mi355x]\n' + text if text else ''))
    return c


def fn(text='', exponential=False):
    from yolo_tf_amd.optim import learning_rate_fn
    return learning_rate_fn(cfg(text, exponential), BASE)


def _as_it_was(config, base_lr):
    """optim.learning_rate_fn before the schedule keys existed, restated."""
    try:
        steps = config.getint('exponential_decay', 'decay_steps')
        rate = config.getfloat('exponential_decay', 'decay_rate')
        staircase = config.getboolean('exponential_decay', 'staircase')
    except (configparser.NoSectionError, configparser.NoOptionError):
        return lambda step: base_lr
    return lambda step: base_lr * rate ** (math.floor(step / steps) if staircase else step / steps)


def test_keys_absent_is_the_function_as_it_was_on_the_shipped_config():
    from yolo_tf_amd.optim import LR_KEYS, learning_rate_fn
    shipped = configparser.ConfigParser()
    assert shipped.read(os.path.join(ROOT, 'config.ini'))
    assert not any(shipped.has_option('mi355x', k) for k in LR_KEYS)                  # (the shipped keys are comments)
    for config in (shipped, cfg(), cfg(exponential=True), cfg('ema_decay = 0.9', exponential=True)):
        new, old = learning_rate_fn(config, 1e-4), _as_it_was(config, 1e-4)
        steps = list(range(0, 300001, 997)) + [1, 99, 100, 101, 199, 200, 300000]
        assert [new(s) for s in steps] == [old(s) for s in steps]                        # the same floats
    assert learning_rate_fn(None, 0.25)(7) == 0.25
    assert fn(exponential=True)(0) == BASE and fn(exponential=True)(100) == BASE * 0.5 and fn(exponential=True)(250) == BASE * 0.25


def test_policy_exponential_and_constant():
    assert [fn('lr_policy = exponential', True)(s) for s in (0, 99, 100, 250)] == [BASE, BASE, BASE * 0.5, BASE * 0.25]
    assert [fn('lr_policy = constant', True)(s) for s in (0, 100, 10 ** 6)] == [BASE] * 3
    assert fn('lr_policy = CONSTANT')(5) == BASE
    with pytest.raises(ValueError, match='lr_policy = exponential'):
        fn('lr_policy = exponential')


def test_policy_steps_switches_at_exactly_the_boundary():
    f = fn('lr_policy = steps\nlr_steps = 40000 60000\nlr_scales = 0.1 0.1')
    assert f(0) == f(39999) == BASE
    assert f(40000) == f(59999) == BASE * 0.1
    assert f(60000) == f(10 ** 7) == BASE * 0.1 * 0.1
    g = fn('lr_policy = steps\nlr_steps = 1, 3\nlr_scales = 0.1, 10')                   # commas, and a scale above 1
    assert [g(s) for s in range(5)] == [BASE, BASE * 0.1, BASE * 0.1, BASE * 0.1 * 10, BASE * 0.1 * 10]
    assert fn('lr_policy = steps')(123) == BASE                                         # no steps: constant


def test_policy_poly():
    f = fn('lr_policy = poly\nlr_max_steps = 1000\nlr_power = 2')
    assert f(0) == BASE and f(500) == BASE * 0.25 and f(1000) == 0.0 and f(5000) == 0.0
    assert f(250) == BASE * (1.0 - 250 / 1000) ** 2.0
    d = fn('lr_policy = poly\nlr_max_steps = 100')                                      # the power defaults to 4
    assert d(0) == BASE and d(50) == BASE * 0.5 ** 4.0 and d(100) == 0.0


def test_policy_cosine_at_the_ends_the_middle_and_beyond():
    f = fn('lr_policy = cosine\nlr_max_steps = 1000')
    assert f(0) == BASE
    assert f(500) == pytest.approx(BASE * 0.5, rel=1e-15)
    assert f(1000) == 0.0 and f(1001) == 0.0 and f(10 ** 6) == 0.0
    assert f(250) == BASE * (0.5 * (1.0 + math.cos(math.pi * 250 / 1000)))
    assert all(f(s) > f(s + 1) for s in range(0, 1000, 37))
    m = fn('lr_policy = cosine\nlr_min_ratio = 0.1\nlr_max_steps = 200')
    assert m(0) == BASE and m(100) == pytest.approx(BASE * 0.55, rel=1e-15) and m(200) == pytest.approx(BASE * 0.1, rel=1e-15) and m(999) == m(200)


def test_burn_in():
    N = 1000
    f = fn('burn_in = %d' % N)                                                           # Darknet's default power, 4; the policy stays the default (constant here)
    assert f(0) == BASE * (1 / N) ** 4.0 and f(0) > 0                                    # step + 1: the first update is not a zero update
    assert f(N - 2) == BASE * ((N - 1) / N) ** 4.0 < BASE
    assert f(N - 1) == BASE and f(N) == BASE and f(10 * N) == BASE
    g = fn('burn_in = 4\nburn_in_power = 1\nlr_policy = steps\nlr_steps = 2\nlr_scales = 0.5')
    assert [g(s) for s in range(6)] == [BASE * 0.25, BASE * 0.5, BASE * 0.5 * 0.75, BASE * 0.5, BASE * 0.5, BASE * 0.5]
    e = fn('burn_in = 200', exponential=True)                                            # on top of [exponential_decay]
    assert e(99) == BASE * (100 / 200) ** 4.0 and e(100) == BASE * 0.5 * (101 / 200) ** 4.0 and e(300) == BASE * 0.125
    assert fn('burn_in = 0', True)(150) == BASE * 0.5
    # what the command-line test runs: --lr_policy steps --lr_steps 1 --lr_scales 0.1 --burn_in 2
    c = fn('lr_policy = steps\nlr_steps = 1\nlr_scales = 0.1\nburn_in = 2')
    assert c(0) == BASE * 0.5 ** 4.0 and c(1) == BASE * 0.1 and c(2) == BASE * 0.1


@pytest.mark.parametrize('text,key', [
    ('lr_policy = steps\nlr_steps = 10 20\nlr_scales = 0.1', 'lr_steps'),
    ('lr_policy = steps\nlr_steps = 10\nlr_scales = 0.1 0.1', 'lr_scales'),
    ('lr_policy = steps\nlr_scales = 0.1', 'lr_scales'),
    ('lr_policy = steps\nlr_steps = 20 10\nlr_scales = 0.1 0.1', 'lr_steps'),
    ('lr_policy = steps\nlr_steps = -5\nlr_scales = 0.1', 'lr_steps'),
    ('lr_policy = steps\nlr_steps = 5\nlr_scales = -0.1', 'lr_scales'),
    ('lr_policy = steps\nlr_steps = soon\nlr_scales = 0.1', 'lr_steps'),
    ('lr_steps = 5\nlr_scales = 0.1', 'lr_steps'),
    ('lr_policy = cosine\nlr_steps = 5\nlr_scales = 0.1', 'lr_steps'),
    ('lr_policy = poly', 'lr_max_steps'),
    ('lr_policy = cosine', 'lr_max_steps'),
    ('lr_policy = cosine\nlr_max_steps = 0', 'lr_max_steps'),
    ('lr_policy = poly\nlr_max_steps = -100', 'lr_max_steps'),
    ('lr_policy = poly\nlr_max_steps = 100\nlr_power = -1', 'lr_power'),
    ('lr_policy = cosine\nlr_max_steps = 100\nlr_min_ratio = -0.5', 'lr_min_ratio'),
    ('lr_policy = cosine\nlr_max_steps = 100\nlr_min_ratio = 1.5', 'lr_min_ratio'),
    ('burn_in = -1', 'burn_in'),
    ('burn_in = 10\nburn_in_power = -4', 'burn_in_power'),
    ('burn_in = 10 20', 'burn_in'),
    ('lr_policy = warmup', 'lr_policy'),
])
def test_errors_name_the_key(text, key):
    with pytest.raises(ValueError, match=key):
        fn(text)
