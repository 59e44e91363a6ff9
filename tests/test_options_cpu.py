"""yolo_tf_amd/options.py, the one table and the one reader of the ``[mi355x]`` keys: every case of tests/golden/option_cases.json.gz (recorded by
scripts/record_option_cases.py from the tree BEFORE the resolvers moved onto the reader) gives the same value -- floats bit for bit -- or the same
exception type and message; the seven keys that were read inline, by hand from the expressions they replace; the table against config.ini; and the
promises of the module: host code only, the only place that spells the section."""
import argparse
import ast
import configparser
import gzip
import importlib.util
import json
import os
import re

import pytest

from yolo_tf_amd import options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location('record_option_cases', os.path.join(ROOT, 'scripts', 'record_option_cases.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RECORDER = _recorder()
with gzip.open(os.path.join(ROOT, 'tests', 'golden', 'option_cases.json.gz'), 'rt') as _f:
    GOLDEN = json.load(_f)
FUNCTIONS = sorted(set(c[0] for c in GOLDEN['cases']))


def _hexed(v):
    """Every float as its float.hex(): equal means bit-equal, NaN included."""
    if isinstance(v, float):
        return {'f': v.hex()}
    if isinstance(v, dict):
        return {k: _hexed(x) for k, x in v.items()}
    return [_hexed(x) for x in v] if isinstance(v, list) else v


def _decode(v):
    if isinstance(v, dict) and set(v) == {'t'}:
        return tuple(_decode(x) for x in v['t'])
    if isinstance(v, dict):
        return {k: _decode(x) for k, x in v.items()}
    return [_decode(x) for x in v] if isinstance(v, list) else v


def test_golden_covers_every_key_and_resolver():
    assert re.match(r'^[0-9a-f]{40}$', GOLDEN['commit'])
    assert len(GOLDEN['cases']) > 1000 and len(FUNCTIONS) == 15
    named = set(k for c in GOLDEN['cases'] if isinstance(c[1], list) and c[1][2] for k in c[1][2])
    inline = {'dtype', 'bucket_mb', 'grad_dtype', 'deterministic', 'comm_cus', 'sync_bn'}        # (no function at the recorded commit: test_inline_keys)
    assert [k for k in options.KEYS if k not in inline and k not in named] == []
    for fn in FUNCTIONS:
        assert fn == 'refuse_recipe' or any(c[0] == fn and c[1] is None for c in GOLDEN['cases']), fn                     # no config
        assert fn == 'refuse_recipe' or any(c[0] == fn and isinstance(c[1], list) and c[1][2] is None for c in GOLDEN['cases']), fn      # no section
    assert any(c[0] == 'learning_rate_fn' and c[1] == 'object' for c in GOLDEN['cases'])   # an object that is no config


# The ONE accepted difference from the recorded commit, case by case: (function, config, arguments) -> (recorded outcome, outcome now).
# The reader takes a None config as a config without keys, so the resolvers that asked ``config.has_section`` / ``config.has_option`` themselves no longer
# raise AttributeError on None: they answer with the defaults (train.recipe_setting still needs [config] model and fails one line later).  And
# train.recipe_setting no longer makes an empty section in a config that has none when the command line gives it nothing to write; no reader can tell
# an empty section from a missing one.
_NO_SECTION, _NO_HAS_SECTION = ['yolo2', False, None], "'NoneType' object has no attribute 'has_section'"
ACCEPTED = [
    ('multiscale.configure', None, {}, {'raises': ['AttributeError', _NO_HAS_SECTION]}, {'value': None}),
    ('tta.options', None, {}, {'raises': ['AttributeError', _NO_HAS_SECTION]}, {'value': {'t': ['', 0.55]}}),
    ('nms_options', None, {}, {'raises': ['AttributeError', "'NoneType' object has no attribute 'has_option'"]}, {'value': {'t': ['hard', 0.5]}}),
    ('train.multiscale_setting', None, {'argv': ['--data', 'synthetic']}, {'raises': ['AttributeError', _NO_HAS_SECTION]}, {'value': None}),
    ('train.recipe_setting', None, {'argv': []}, {'raises': ['AttributeError', _NO_HAS_SECTION]}, {'raises': ['AttributeError', "'NoneType' object has no attribute 'get'"]}),
    ('train.recipe_setting', _NO_SECTION, {'argv': []}, {'value': [{'t': [1, 0.0, 'l2']}, {}]}, {'value': [{'t': [1, 0.0, 'l2']}, None]}),
]


@pytest.mark.parametrize('fn', FUNCTIONS)
def test_replay(fn):
    """Equal outcomes: the JSON form of the value with every float as its float.hex(), or the exception's type name and exact message -- but for the
    cases of ACCEPTED, which must be recorded as listed there and must now give what is listed there."""
    accepted = {json.dumps(c[:3]): c[3:] for c in ACCEPTED if c[0] == fn}
    mismatches, met = [], 0
    for name, config, a, want in GOLDEN['cases']:
        if name == fn:
            got = RECORDER.outcome(name, config, _decode(a))
            recorded, now = accepted.get(json.dumps([name, config, a]), (want, want))
            met += recorded is not want
            if _hexed(want) != _hexed(recorded) or _hexed(got) != _hexed(now):
                mismatches.append((config, a, want, got))
    assert mismatches == [], '%d of the cases of %s differ, the first: %r' % (len(mismatches), fn, mismatches[0])
    assert met == len(accepted)


def test_every_resolver_takes_no_config():
    """What each resolver answers to a None config now, spelled out (the golden record holds what it answered before)."""
    import train
    from yolo_tf_amd import multiscale, session, tta, utils
    from yolo_tf_amd.optim import learning_rate_fn
    from yolo_tf_amd.utils import augment
    assert multiscale.configure(None) is None and train.multiscale_setting(train.make_args(['--data', 'synthetic']), None) is None
    assert tta.options(None) == ('', 0.55) and utils.nms_options(argparse.Namespace(), None) == ('hard', 0.5)
    assert session.ema_decay_option(None, None) == 0.0 and session.box_loss_option(None, None) == 'mse' and session.recipe_options(None) == (1, 0.0, 'l2')
    assert session.loss_options(None) == session.LOSS_OPTION_DEFAULTS and augment.compose_options(None) == augment.COMPOSE_DEFAULTS
    assert learning_rate_fn(None, 0.5)(1000) == 0.5
    assert train.compose_setting(train.make_args([]), None) is None and train.box_loss_setting(train.make_args([]), None) == 'mse'
    assert train.loss_setting(train.make_args([]), None) == session.LOSS_OPTION_DEFAULTS
    with pytest.raises(AttributeError):          # [config] model decides the YOLO (v1) refusals: that needs a config
        train.recipe_setting(train.make_args([]), None)


def _config(text=None):
    c = configparser.ConfigParser()
    c.read_string('[config]\nmodel = yolo2\n' + ('' if text is None else '[mi355x]\n' + text))
    return c


# What the expressions that train.py, detect.py, eval.py and TrainSession.__init__ spelled inline gave, by hand:
#   dtype           args.dtype or (config.get(S, 'dtype') if config.has_option(S, 'dtype') else 'bf16')
#   bucket_mb       config.getfloat(S, 'bucket_mb') if config.has_option(S, 'bucket_mb') else 64.0
#   grad_dtype      config.get(S, 'grad_dtype') if config.has_option(S, 'grad_dtype') else 'f32'
#   sync_bn         config.getboolean(S, 'sync_bn') if config.has_option(S, 'sync_bn') else False          (shard_optimizer alike)
#   deterministic   cfg is not None and cfg.has_option(S, 'deterministic') and cfg.getboolean(S, 'deterministic')      (then: or YOLO2_DETERMINISTIC == '1')
#   comm_cus        comm_cus if comm_cus is not None else (cfg.getint(S, 'comm_cus') if cfg is not None and cfg.has_option(S, 'comm_cus') else 32)
INLINE = [
    ('dtype', None, None, 'bf16'), ('dtype', '', None, 'bf16'), ('dtype', 'dtype = bf16', None, 'bf16'), ('dtype', 'dtype = f32', None, 'f32'),
    ('dtype', 'dtype = int8', None, 'int8'), ('dtype', 'dtype = fp8', None, 'fp8'), ('dtype', 'dtype = f32', 'bf16', 'bf16'), ('dtype', 'dtype = bf16', 'f32', 'f32'),
    ('bucket_mb', None, None, 64.0), ('bucket_mb', '', None, 64.0), ('bucket_mb', 'bucket_mb = 64', None, 64.0), ('bucket_mb', 'bucket_mb = 0.5', None, 0.5),
    ('bucket_mb', 'bucket_mb = -1', None, -1.0), ('bucket_mb', 'bucket_mb = abc', None, ValueError("could not convert string to float: 'abc'")),
    ('grad_dtype', None, None, 'f32'), ('grad_dtype', '', None, 'f32'), ('grad_dtype', 'grad_dtype = f32', None, 'f32'), ('grad_dtype', 'grad_dtype = bf16', None, 'bf16'),
    ('grad_dtype', 'grad_dtype = BF16', None, 'BF16'),
    ('comm_cus', None, None, 32), ('comm_cus', '', None, 32), ('comm_cus', 'comm_cus = 32', None, 32), ('comm_cus', 'comm_cus = 0', None, 0), ('comm_cus', 'comm_cus = -4', None, -4),
    ('comm_cus', 'comm_cus = 16', 32, 32), ('comm_cus', 'comm_cus = 16', 0, 0), ('comm_cus', 'comm_cus = x', 8, 8),
    ('comm_cus', 'comm_cus = x', None, ValueError("invalid literal for int() with base 10: 'x'")),
    ('comm_cus', 'comm_cus = 1.5', None, ValueError("invalid literal for int() with base 10: '1.5'")),
]
for _key in ('sync_bn', 'shard_optimizer', 'deterministic'):
    INLINE += [(_key, None, None, False), (_key, '', None, False), (_key, '%s = maybe' % _key, None, ValueError('Not a boolean: maybe'))]
    INLINE += [(_key, '%s = %s' % (_key, text), None, value) for text, value in (('0', False), ('1', True), ('false', False), ('true', True), ('no', False), ('Yes', True),
                                                                                   ('off', False), ('ON', True))]


@pytest.mark.parametrize('key,text,given,want', INLINE)
def test_inline_keys(key, text, given, want):
    for config in ([None, configparser.ConfigParser(), _config()] if text is None else [_config(text)]):      # text None: no config, no section, an empty section
        if isinstance(want, Exception):
            with pytest.raises(type(want)) as e:
                options.read(config, key, given)
            assert str(e.value) == str(want)
        else:
            got = options.read(config, key, given)
            assert got == want and type(got) is type(want)


def test_reader():
    cfg = _config('ema_decay = 0.5\nlr_steps = 10, 20 30\nmosaic_scale = 0.25 2\nburn_in = 7,\nrescore = maybe\n')
    assert options.read(cfg, 'ema_decay') == 0.5 and options.read(cfg, 'ema_decay', 0.0) == 0.0 and options.read(cfg, 'ema_decay', how='text') == '0.5'
    assert options.read(cfg, 'lr_steps') == [10, 20, 30] and options.read(cfg, 'mosaic_scale') == [0.25, 2.0] and options.read(cfg, 'lr_scales') == ()
    assert options.read(cfg, 'burn_in', how='list') == [7] and options.read(cfg, 'burn_in_power', how='list') == 4.0
    with pytest.raises(ValueError) as e:
        options.read(cfg, 'burn_in')
    assert str(e.value) == "invalid literal for int() with base 10: '7,'"
    with pytest.raises(ValueError) as e:
        options.read(cfg, 'rescore', invalid='true or false')
    assert str(e.value) == "[mi355x] rescore = 'maybe': true or false" == str(options.refusal(cfg, 'rescore', 'true or false'))
    for none in (None, object(), {}, configparser.ConfigParser()):
        assert not options.has(none, 'nms') and options.read(none, 'nms') == 'hard' and options.read(none, 'nms', 'linear') == 'linear'
    with pytest.raises(KeyError):
        options.read(cfg, 'no_such_key')
    with pytest.raises(KeyError):
        options.has(None, 'no_such_key')


def test_write():
    cfg = configparser.ConfigParser()
    args = argparse.Namespace(mosaic=None, mixup=0.5, accum_steps=4, weight_decay=0.0005, weight_decay_mode='l2', lr_steps=['3', '6'], lr_scales=None)
    options.write(cfg, args, ('mosaic', 'lr_scales'))
    assert not cfg.has_section('mi355x')                               # nothing given: nothing written, no section made
    options.write(cfg, args, ('mosaic', 'mixup', 'accum_steps', 'weight_decay', 'weight_decay_mode', 'lr_steps', 'lr_scales'))
    assert dict(cfg.items('mi355x')) == {'mixup': '0.5', 'accum_steps': '4', 'weight_decay': '0.0005', 'weight_decay_mode': 'l2', 'lr_steps': '3 6'}
    assert options.read(cfg, 'mixup') == 0.5 and options.read(cfg, 'lr_steps') == [3, 6]


def test_table_against_config_ini():
    """Every key of the table is named in config.ini's [mi355x] section, set or as a ``;`` comment line, and the file sets no key the table lacks."""
    with open(os.path.join(ROOT, 'config.ini')) as f:
        text = f.read()
    section = text[text.index('\n[mi355x]'):text.index('\n[summary]')]
    named = set(re.findall(r'^;? ?(\w+) = ', section, re.M))
    assert [k for k in options.KEYS if k not in named] == []
    cfg = configparser.ConfigParser()
    cfg.read_string(text)
    assert [k for k in cfg.options('mi355x') if k not in options.KEYS] == []
    for key in cfg.options('mi355x'):                                   # what the shipped file sets reads as the table's default
        assert options.read(cfg, key) == options.KEYS[key].default, key
    for k in options.KEYS.values():
        assert k.kind in ('bool', 'int', 'float', 'choice', 'ints', 'floats', 'text') and k.meaning and (k.kind == 'choice') == (k.choices is not None), k.name


def test_single_source():
    """options.py is host code without torch or the library; nothing else in the non-test Python spells the section (bench.py aside, which no pull
    request edits, and the recorder, which has to run on a tree without options.py); a session class resolves its config object once."""
    with open(os.path.join(ROOT, 'yolo_tf_amd', 'options.py')) as f:
        tree = ast.parse(f.read())
    imported = [n.names[0].name if isinstance(n, ast.Import) else n.module for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert imported == ['collections']
    spelled = []
    for top, dirs, files in [(ROOT, [], os.listdir(ROOT))] + [found for d in ('yolo_tf_amd', 'scripts', 'oracle') for found in os.walk(os.path.join(ROOT, d))]:
        for name in files:
            path = os.path.relpath(os.path.join(top, name), ROOT)
            if name.endswith('.py') and path not in ('bench.py', os.path.join('yolo_tf_amd', 'options.py'), os.path.join('scripts', 'record_option_cases.py')):
                with open(os.path.join(top, name)) as f:
                    if re.search(r'''['"]mi355x['"]''', f.read()):
                        spelled.append(path)
    assert spelled == []
    with open(os.path.join(ROOT, 'yolo_tf_amd', 'session.py')) as f:
        session = f.read()
    for cls in re.split(r'^class ', session, flags=re.M)[1:]:
        assert cls.count('config if config is not None else') <= 1, cls[:40]


def test_add_flags():
    """The flags of train.py, detect.py and eval.py that the table makes: names, types, choices and the None default that lets the key decide."""
    parser = argparse.ArgumentParser()
    options.add_flags(parser, ('nms', ('sigma', 'nms_sigma'), 'tta', 'accum_steps', 'lr_steps', 'lr_scales', 'weight_decay_mode'))
    assert vars(parser.parse_args([])) == dict(nms=None, sigma=None, tta=None, accum_steps=None, lr_steps=None, lr_scales=None, weight_decay_mode=None)
    got = parser.parse_args(['--nms', 'linear', '--sigma', '0.25', '--tta', 'flip 320', '--accum_steps', '4', '--lr_steps', '3', '6', '--lr_scales', '0.5', '0.5'])
    assert (got.nms, got.sigma, got.tta, got.accum_steps, got.lr_steps, got.lr_scales) == ('linear', 0.25, 'flip 320', 4, ['3', '6'], ['0.5', '0.5'])
    for bad in (['--nms', 'softer'], ['--accum_steps', '2.5'], ['--weight_decay_mode', 'adamw'], ['--sigma', 'x']):
        with pytest.raises(SystemExit):
            parser.parse_args(bad)
    import detect
    import eval as eval_cli
    import train
    a = train.make_args([])
    assert all(getattr(a, k) is None for k in ('multiscale', 'multiscale_every', 'mosaic', 'mixup', 'box_loss', 'class_loss', 'ignore_thresh', 'rescore', 'label_smoothing',
                                                 'focal_gamma', 'accum_steps', 'weight_decay', 'weight_decay_mode', 'lr_policy', 'burn_in', 'lr_steps', 'lr_scales', 'dtype'))
    a = train.make_args(['--multiscale', '', '--multiscale_every', '5', '--mosaic', '0.5', '--box_loss', 'ciou', '--no_rescore', '--lr_policy', 'steps', '--burn_in', '3'])
    assert (a.multiscale, a.multiscale_every, a.mosaic, a.box_loss, a.rescore, a.lr_policy, a.burn_in) == ('', 5, 0.5, 'ciou', False, 'steps', 3)
    for cli, argv in ((detect, ['x.jpg']), (eval_cli, [])):
        a = cli.make_args(argv)
        assert (a.nms, a.sigma, a.tta, a.tta_iou) == (None, None, None, None)
        a = cli.make_args(argv + ['--nms', 'gaussian', '--sigma', '0.5', '--tta', 'flip', '--tta_iou', '0.6'])
        assert (a.nms, a.sigma, a.tta, a.tta_iou) == ('gaussian', 0.5, 'flip', 0.6)
