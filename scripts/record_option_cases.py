"""Records what every resolver of the ``[mi355x]`` options returns or refuses for a table of configs and arguments: tests/golden/option_cases.json.gz.

    python scripts/record_option_cases.py [--out tests/golden/option_cases.json.gz] [--commit NAME]

Pure host work: no device is touched.  Only names that scripts and tests import are called (the resolvers of session, optim, multiscale, tta,
utils.augment and utils, and train.py's ``*_setting`` functions), so the same script runs on the tree before and after a change of the option plumbing.
Run it on the PARENT of a pull request that moves that plumbing; tests/test_options_cpu.py replays every case against the checkout.  A case is
[function, config, arguments, outcome]: the config is null (no config), "object" (an object that is no config) or [model, decay, keys] -- the
family of [config] model, whether [exponential_decay] is there, and the keys of the section (null: no section) -- of which ``make_config`` makes the INI text;
the outcome is {"value": ...} with every tuple as {"t": [...]} (the arguments are written the same way; a float is written as Python's repr, which reads back
bit for bit, NaN and Infinity as json writes them), or {"raises": [type name, message]}.  The header names the commit."""
import argparse
import configparser
import gzip
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASE = '[config]\nmodel = %s\n[yolo]\ninference = tiny\nwidth = 448\nheight = 448\n[yolo2]\ninference = tiny\nwidth = 416\nheight = 416\n'
DECAY = '[exponential_decay]\ndecay_steps = 100\ndecay_rate = 0.5\nstaircase = true\n'


def ini(keys=None, model='yolo2', section=True, decay=False):
    """A config as a case holds it: [model, decay, keys]; ``section`` False leaves the section out altogether."""
    return [model, decay, dict(keys or {}) if section else None]


def make_config(spec):
    """None, an object that is no config, or the ConfigParser of [model, decay, keys]: the sections every resolver may look at, [exponential_decay] on
    request, and ``[mi355x]`` with the keys."""
    if spec is None or isinstance(spec, configparser.ConfigParser):
        return spec
    if spec == 'object':
        return object()
    model, decay, keys = spec
    config = configparser.ConfigParser()
    config.read_string(BASE % model + (DECAY if decay else '') + ('' if keys is None else '[mi355x]\n' + ''.join('%s = %s\n' % kv for kv in keys.items())))
    return config


def encode(v):
    if isinstance(v, bool) or v is None or isinstance(v, (int, float, str)):
        return v
    if isinstance(v, dict):
        return {str(k): encode(x) for k, x in v.items()}
    if isinstance(v, tuple):
        return {'t': [encode(x) for x in v]}
    if isinstance(v, list):
        return [encode(x) for x in v]
    return encode(v.item())           # a numpy scalar


def section_of(config):
    """The keys a ``*_setting`` function left in the config: a dict, empty for a section without keys, or None where there is no section (or no config)."""
    return dict(config.items('mi355x')) if config is not None and config.has_section('mi355x') else None


def lr_steps(config):
    """0, 1 and N - 1, N, N + 1 around every breakpoint the config (a case's, or a ConfigParser) names: lr_steps, burn_in, lr_max_steps (so lr_max_steps + 1 is
    among them) and decay_steps."""
    points = {100}
    config = make_config(config)
    if isinstance(config, configparser.ConfigParser):
        for section, key in (('mi355x', 'lr_steps'), ('mi355x', 'burn_in'), ('mi355x', 'lr_max_steps'), ('exponential_decay', 'decay_steps')):
            if config.has_option(section, key):
                for token in config.get(section, key).replace(',', ' ').split():
                    try:
                        points.add(int(token))
                    except ValueError:
                        pass
    steps = {0, 1}
    for n in points:
        steps |= {n - 1, n, n + 1}
    return sorted(s for s in steps if 0 <= s < 2 ** 40)


def call(fn, config, a):
    """Runs resolver ``fn`` (the first field of a case) on a fresh config made of ``config`` with the arguments ``a`` (a dict)."""
    import train
    from yolo_tf_amd import multiscale, optim, session, tta, utils
    from yolo_tf_amd.utils import augment
    cfg = make_config(config)
    if fn == 'ema_decay_option':
        return session.ema_decay_option(a.get('ema_decay'), cfg)
    if fn == 'box_loss_option':
        return session.box_loss_option(a.get('box_loss'), cfg)
    if fn == 'loss_options':
        options = session.loss_options(cfg, **a)
        return [options, session.loss_options_set(options)]
    if fn == 'recipe_options':
        return session.recipe_options(cfg, **a)
    if fn == 'refuse_recipe':
        return session.refuse_recipe(**a)
    if fn == 'learning_rate_fn':
        rate = optim.learning_rate_fn(cfg, a['base_lr'])
        return [[s, rate(s)] for s in a['steps']]
    if fn == 'multiscale.configure':
        return multiscale.configure(cfg, a.get('spec'), a.get('every'))
    if fn == 'tta.options':
        return tta.options(cfg, a.get('spec'), a.get('iou'))
    if fn == 'compose_options':
        return augment.compose_options(cfg)
    if fn == 'nms_options':
        return utils.nms_options(argparse.Namespace(**a), cfg)
    if fn.startswith('train.'):
        args = train.make_args(a['argv'])
        value = getattr(train, fn[len('train.'):])(args, cfg)
        # (both write the command line into the config, where the input pipeline and the session's learning_rate_fn read it: the section belongs to the outcome)
        return [value, section_of(cfg)] if fn in ('train.compose_setting', 'train.recipe_setting') else value
    raise KeyError(fn)


def outcome(fn, config, a):
    try:
        return {'value': encode(call(fn, config, a))}
    except Exception as e:       # noqa: BLE001  (the refusal is the record)
        return {'raises': [type(e).__name__, str(e)]}


def cases():
    out = []
    add = lambda fn, config, **a: out.append((fn, config, a))

    def sweep(fn, key, texts, context=None, given=None, **a):
        """``key`` absent and at every text of ``texts``, the other keys at ``context``; then every value of ``given`` as the argument over the key at
        texts[1] (by convention a valid value that is on and is not the default), the first one over the key absent too."""
        context = context or {}
        add(fn, ini(context), **a)
        for text in texts:
            add(fn, ini(dict(context, **{key: text})), **a)
        for name, values in (given or {}).items():
            add(fn, ini(context), **dict(a, **{name: values[0]}))
            for value in values:
                add(fn, ini(dict(context, **{key: texts[1]})), **dict(a, **{name: value}))

    for fn, a in (('ema_decay_option', {}), ('box_loss_option', {}), ('loss_options', {}), ('recipe_options', {}), ('compose_options', {}),
                  ('learning_rate_fn', dict(base_lr=1e-3, steps=[0, 1, 99, 100, 101]))):
        add(fn, None, **a)                           # no config at all
        add(fn, ini(section=False), **a)             # a config without the section
    add('learning_rate_fn', 'object', base_lr=1e-3, steps=[0, 1, 7])
    add('learning_rate_fn', ini(section=False, decay=True), base_lr=1e-3, steps=[0, 1, 99, 100, 101, 200])
    for fn, a in (('multiscale.configure', {}), ('tta.options', {}), ('nms_options', {}), ('train.multiscale_setting', dict(argv=['--data', 'synthetic'])),
                  ('train.compose_setting', dict(argv=[])), ('train.box_loss_setting', dict(argv=[])), ('train.loss_setting', dict(argv=[])),
                  ('train.recipe_setting', dict(argv=[]))):
        add(fn, None, **a)                           # no config at all
        add(fn, ini(section=False), **a)             # a config without the section

    # --- session: ema_decay, box_loss, the loss options, the recipe ---
    sweep('ema_decay_option', 'ema_decay', ['0', '0.9', '0.0', '0.999999', '0.9999999999999999', '1', '1.0', '-0.001', '-0.0', 'abc', 'nan', '0.5,', '1e-3'],
          given=dict(ema_decay=[0.5, 0.0, 0, 1.0, -0.5, 'abc', '0.25', float('nan')]))
    sweep('box_loss_option', 'box_loss', ['mse', 'giou', 'iou', 'diou', 'ciou', 'GIoU', 'l1', 'mse giou'], given=dict(box_loss=['mse', 'ciou', 'DIoU', ' iou ', 'l2', 0]))
    sweep('loss_options', 'box_loss', ['mse', 'giou', 'ciou', 'l1'], given=dict(box_loss=['mse', 'ciou', 'l2']))
    sweep('loss_options', 'class_loss', ['mse', 'ce', 'focal', 'CE', ' Focal', 'bogus'], given=dict(class_loss=['mse', 'focal', 'FOCAL', 'hinge', 0]))
    sweep('loss_options', 'ignore_thresh', ['0', '0.6', '0.0', '1e-9', '0.999999', '1', '1.0', '-0.1', '-0.0', 'abc', 'nan', 'inf', '0.6,'],
          given=dict(ignore_thresh=[0.0, 0.7, 0, 1.0, -0.1, 'abc', '0.5', float('nan')]))
    sweep('loss_options', 'rescore', ['false', 'true', '0', '1', 'yes', 'no', 'on', 'off', 'True', 'maybe', '2'], given=dict(rescore=[False, True, 0, 1, 2, 'true', 0.0]))
    sweep('loss_options', 'label_smoothing', ['0', '0.1', '0.0', '0.999999', '1', '1.0', '-0.1', 'abc', 'nan'], context=dict(class_loss='ce'),
          given=dict(label_smoothing=[0.0, 0.2, 1.0, -0.1, 'abc']))
    sweep('loss_options', 'focal_gamma', ['2', '3', '0', '1', '1.0', '0.5', '0.999999', '-1', 'inf', '1e30', 'abc', 'nan'], context=dict(class_loss='focal'),
          given=dict(focal_gamma=[2.0, 0.0, 1.0, 0.5, -1.0, float('inf'), 'abc']))
    for cls in ('focal', 'mse'):          # smoothing belongs to ce and focal; focal_gamma is read, but held to its range with focal only
        sweep('loss_options', 'label_smoothing', ['0', '0.1', '1', 'abc'], context=dict(class_loss=cls), given=dict(label_smoothing=[0.0, 0.2]))
    for cls in ('ce', 'mse'):
        sweep('loss_options', 'focal_gamma', ['2', '0.5', '-1', 'abc'], context=dict(class_loss=cls), given=dict(focal_gamma=[2.0, 0.5]))
    add('loss_options', ini(dict(class_loss='ce', label_smoothing='0.1')), class_loss='mse')                 # smoothing left on under an argument that takes its class term away
    add('loss_options', ini(dict(label_smoothing='0.1')), class_loss='ce')
    add('loss_options', ini(dict(class_loss='bogus', ignore_thresh='7', box_loss='l1')))                     # several refusals: the first one speaks
    add('loss_options', ini(dict(class_loss='focal', ignore_thresh='0.6', rescore='true', label_smoothing='0.1', focal_gamma='3', box_loss='ciou')))
    add('loss_options', ini(dict(class_loss='focal', ignore_thresh='0.6', rescore='true', label_smoothing='0.1', focal_gamma='3', box_loss='ciou')),
        box_loss='mse', class_loss='mse', ignore_thresh=0.0, rescore=False, label_smoothing=0.0, focal_gamma=2.0)
    sweep('recipe_options', 'accum_steps', ['1', '4', ' 8 ', '0', '-1', '2.5', 'abc', '1e1', '4,'], given=dict(accum_steps=[1, 2, 0, -3, '4', 'abc', 2.0, True]))
    sweep('recipe_options', 'weight_decay', ['0', '0.0005', '0.0', '1e30', '-1', '-0.0', 'inf', 'nan', 'abc', '5e-4,'],
          given=dict(weight_decay=[0.0, 0.001, 0, -1.0, float('inf'), 'abc', '0.01']))
    sweep('recipe_options', 'weight_decay_mode', ['l2', 'decoupled', 'Decoupled', ' L2 ', 'adamw'], given=dict(weight_decay_mode=['l2', 'decoupled', 'DECOUPLED', 'adamw', 0]))
    add('recipe_options', ini(dict(accum_steps='0', weight_decay='-1', weight_decay_mode='adamw')))
    for accum, decay, mode, v1, shard, opt in ((1, 0.0, 'l2', False, False, 'adam'), (1, 0.0, 'l2', True, True, 'ftrl'), (2, 0.0, 'l2', True, False, 'adam'),
                                                 (2, 0.0, 'l2', False, True, 'adam'), (1, 0.0005, 'l2', False, True, 'adam'), (4, 0.0005, 'l2', False, True, 'adam'),
                                                 (1, 0.0005, 'l2', True, False, 'adam'), (1, 0.0005, 'decoupled', False, False, 'ftrl'),
                                                 (1, 0.0005, 'l2', False, False, 'ftrl'), (1, 0.0, 'decoupled', False, False, 'ftrl'),
                                                 (1, 0.0005, 'decoupled', False, False, 'adam'), (4, 0.0005, 'decoupled', True, True, 'ftrl')):
        add('refuse_recipe', None, accum_steps=accum, weight_decay=decay, weight_decay_mode=mode, v1=v1, shard_optimizer=shard, optimizer=opt)

    # --- optim.learning_rate_fn ---
    def lr(keys, decay=False, base_lr=1e-3):
        config = ini(keys, decay=decay)
        add('learning_rate_fn', config, base_lr=base_lr, steps=lr_steps(config))
    for decay in (False, True):
        lr({}, decay)
        for policy in ('exponential', 'constant', 'steps', 'poly', 'cosine', 'Cosine', ' steps ', 'linear', ''):
            lr(dict(lr_policy=policy), decay)
            if decay:
                lr(dict(lr_policy=policy, lr_max_steps='1000'), decay)
        lr(dict(burn_in='10'), decay)
        lr(dict(lr_steps='10 20', lr_scales='0.1 0.1'), decay)                # lr_steps without the policy steps
        lr(dict(lr_scales='0.1'), decay)
        lr(dict(lr_policy='poly', lr_steps='10', lr_scales='0.1', lr_max_steps='100'), decay)
    for steps, scales in (('10 20', '0.1 0.1'), ('10, 20', '0.1, 0.5'), ('10', '0.1 0.1'), ('10 20', '0.1'), ('20 10', '0.1 0.1'), ('10 10', '0.5 0.5'), ('0', '2'),
                          ('', ''), ('10 x', '0.1 0.1'), ('10 20', '0.1 y'), ('1.5', '0.1'), ('-10', '0.1'), ('10', '-0.1'), ('40000 60000', '0.1 0.1')):
        lr(dict(lr_policy='steps', lr_steps=steps, lr_scales=scales))
    lr(dict(lr_policy='steps'))
    lr(dict(lr_policy='steps', lr_steps='10'))
    lr(dict(lr_policy='steps', lr_scales='0.1'))
    for top in ('100', '1', '0', '-5', 'abc', '100 200', '100,', '1.5', ''):
        lr(dict(lr_policy='poly', lr_max_steps=top))
        lr(dict(lr_policy='cosine', lr_max_steps=top))
    for power in ('4', '1', '0', '0.5', '-1', 'abc', '1 2'):
        lr(dict(lr_policy='poly', lr_max_steps='50', lr_power=power))
    lr(dict(lr_policy='cosine', lr_max_steps='50', lr_power='abc'))              # (a key the policy does not read)
    lr(dict(lr_policy='poly', lr_max_steps='50', lr_min_ratio='2'))
    for ratio in ('0', '0.1', '1', '1.0', '1.000001', '2', '-0.1', 'abc', '0.1 0.2'):
        lr(dict(lr_policy='cosine', lr_max_steps='50', lr_min_ratio=ratio))
    for burn in ('0', '1', '10', '1000', '-1', 'abc', '10 20', '2.5'):
        lr(dict(lr_policy='constant', burn_in=burn))
    lr(dict(burn_in='10'), decay=True)
    for power in ('4', '1', '0', '0.5', '-1', 'abc', '1 2'):
        lr(dict(burn_in='10', burn_in_power=power))
        lr(dict(burn_in_power=power))
    lr(dict(lr_policy='steps', lr_steps='10 20', lr_scales='0.1 0.1', burn_in='15', burn_in_power='2'), base_lr=0.25)
    lr(dict(lr_policy='cosine', lr_max_steps='40', lr_min_ratio='0.05', burn_in='5'), base_lr=1e-4)
    lr(dict(lr_policy='exponential', burn_in='5'), decay=True)

    # --- multiscale.configure, tta.options, utils.nms_options, augment.compose_options ---
    sweep('multiscale.configure', 'multiscale', ['', '320-608', '416', '320 352x352, 608', '100', '320x416 416x320', 'abc', '608-320', '320-600', '   '],
          given=dict(spec=['', '320 416', '96', '100']))
    sweep('multiscale.configure', 'multiscale_every', ['10', '4', '1', '0', '-1', 'abc', '2.5'], context=dict(multiscale='320-608'), given=dict(every=[10, 1, 0, -2]))
    add('multiscale.configure', ini(dict(multiscale_every='0')))                     # (read only when a list is given)
    add('multiscale.configure', ini(dict(multiscale='320-608'), model='yolo'))
    add('multiscale.configure', ini(model='yolo'), spec='448')
    add('multiscale.configure', ini(dict(multiscale='320-608'), model='yolo'), spec='')
    sweep('tta.options', 'tta', ['', 'flip', 'flip 320 608', 'bogus'], given=dict(spec=['', 'flip', '320']))
    sweep('tta.options', 'tta_iou', ['0.55', '0.6', '0', '1', '-5', '7', 'inf', '-inf', 'nan', 'abc', '0.6,'], given=dict(iou=[0.55, 0.7, 0, float('inf'), float('nan'), 'abc', '0.5']))
    sweep('nms_options', 'nms', ['hard', 'linear', 'gaussian', 'Linear', 'softer', ''], given=dict(nms=['hard', 'gaussian', 'softer', '']))
    sweep('nms_options', 'nms_sigma', ['0.5', '0.25', '0', '-1', 'inf', 'abc', '0.25,'], given=dict(sigma=[0.5, 1.0, 0, 0.0, -1.0, '0.3']))
    add('nms_options', ini(dict(nms='linear', nms_sigma='0.25')), nms=None, sigma=None)
    add('nms_options', ini(dict(nms='linear', nms_sigma='0.25')), nms='gaussian', sigma=0.75)
    probability = ['0', '0.5', '0.0', '1', '1.0', '1.000001', '-0.1', '-0.0', 'abc', 'nan', 'inf', '0.5 0.5', '0.5,', '']
    for key, texts in (('mosaic', probability), ('mixup', probability),
                       ('mosaic_scale', ['0.5 1.5', '0.25 2', '1 1', '1, 1', '0 1', '1e-9 1', '2 1', '-1 1', '1', '1 2 3', 'a b', 'nan 1', '1 inf', '']),
                       ('mosaic_center', ['0.25', '0.1', '0', '0.5', '0.500001', '-0.1', 'abc', 'nan', '0.1 0.2']),
                       ('mosaic_min_visible', ['0.25', '0.5', '0', '1', '1.000001', '-0.1', 'abc', 'nan', '0.1 0.2']),
                       ('mosaic_fill', ['114', '0', '0.0', '255', '255.5', '-1', 'abc', 'inf', '1 2']),
                       ('mixup_alpha', ['1.5', '0.5', '1e-9', '0', '-1', '1e30', 'inf', 'abc', '1 2'])):
        sweep('compose_options', key, texts)
    add('compose_options', ini(dict(mosaic='2', mixup='3', mosaic_scale='x')))
    add('compose_options', ini(dict(mixup='3', mosaic_scale='x', mixup_alpha='0')))
    add('compose_options', ini(dict(mosaic='0.5', mosaic_scale='0.25 2', mosaic_center='0.1', mosaic_min_visible='0.5', mosaic_fill='0', mixup='0.1', mixup_alpha='8')))

    # --- train.py: the command line over the keys ---
    train = lambda name, keys, argv, model='yolo2', decay=False: add('train.' + name, ini(keys, model=model, decay=decay), argv=argv)
    for keys in ({}, dict(multiscale='320-608', multiscale_every='4')):
        for argv in ([], ['--multiscale', ''], ['--multiscale', '320 416'], ['--multiscale_every', '1'], ['--multiscale_every', '10'], ['--multiscale_every', '0'],
                     ['--multiscale', '100'], ['--multiscale', '320x416 416x320']):
            train('multiscale_setting', keys, ['--data', 'synthetic'] + argv)
    train('multiscale_setting', dict(multiscale='320-608'), ['--data', 'synthetic'], model='yolo')
    train('multiscale_setting', {}, ['--data', 'cache', '--multiscale', '448'], model='yolo')
    for keys in ({}, dict(mosaic='0.5'), dict(mixup='0.25', mixup_alpha='2'), dict(mosaic='2')):
        for argv in ([], ['--mosaic', '0'], ['--mosaic', '1'], ['--mixup', '0'], ['--mixup', '0.5'], ['--mosaic', '0', '--mixup', '0'], ['--mosaic', '1.5'], ['--mixup', '-1']):
            train('compose_setting', keys, ['--data', 'cache'] + argv)
            if len(argv) < 3:
                train('compose_setting', keys, ['--data', 'synthetic'] + argv[:2])          # (data without raw objects)
    for model in ('yolo2', 'yolo'):
        for keys in ({}, dict(box_loss='giou'), dict(box_loss='mse'), dict(box_loss='l1')):
            for argv in ([], ['--box_loss', 'mse'], ['--box_loss', 'ciou']):
                train('box_loss_setting', keys, argv, model=model)
                train('loss_setting', keys, argv, model=model)
        for keys in ({}, dict(class_loss='focal', ignore_thresh='0.6', rescore='true', label_smoothing='0.1', focal_gamma='3'), dict(class_loss='ce'), dict(rescore='true'),
                     dict(ignore_thresh='0.6'), dict(label_smoothing='0.1'), dict(focal_gamma='0.5'), dict(box_loss='giou', class_loss='bogus'), dict(class_loss='bogus')):
            for argv in ([], ['--class_loss', 'mse'], ['--class_loss', 'ce'], ['--class_loss', 'focal', '--focal_gamma', '0.5'], ['--ignore_thresh', '0'], ['--ignore_thresh', '0.7'],
                         ['--rescore'], ['--no_rescore'], ['--label_smoothing', '0'], ['--label_smoothing', '0.2'], ['--focal_gamma', '2'], ['--focal_gamma', '0.5'],
                         ['--class_loss', 'mse', '--ignore_thresh', '0', '--no_rescore', '--label_smoothing', '0', '--focal_gamma', '2', '--box_loss', 'mse']):
                if len(keys) != 1 or not argv or argv[0] in ('--class_loss', '--no_rescore'):        # (every flag over three configs, the class term and rescore over all)
                    train('loss_setting', keys, argv, model=model)
    recipes = ({}, dict(accum_steps='4', weight_decay='0.0005', weight_decay_mode='decoupled'), dict(shard_optimizer='true'), dict(shard_optimizer='true', accum_steps='2'),
               dict(shard_optimizer='maybe'), dict(lr_policy='steps', lr_steps='10 20', lr_scales='0.1 0.1', burn_in='5'), dict(lr_policy='poly'), dict(lr_policy='cosine', lr_max_steps='30'),
               dict(burn_in='7', burn_in_power='2'), dict(accum_steps='0'), dict(lr_policy='bogus'), dict(lr_steps='10', lr_scales='0.5'))
    for keys in recipes:
        for argv in ([], ['--accum_steps', '1'], ['--accum_steps', '2'], ['--weight_decay', '0'], ['--weight_decay', '0.001'], ['--weight_decay_mode', 'l2'],
                     ['--weight_decay', '0.001', '--weight_decay_mode', 'decoupled', '-o', 'ftrl'], ['--weight_decay', '0.001', '-o', 'ftrl'],
                     ['--lr_policy', 'constant'], ['--lr_policy', 'steps'], ['--lr_policy', 'steps', '--lr_steps', '3', '6', '--lr_scales', '0.5', '0.5'],
                     ['--lr_steps', '3', '6', '--lr_scales', '0.5'], ['--lr_steps', '6', '3', '--lr_scales', '0.5', '0.5', '--lr_policy', 'steps'],
                     ['--lr_policy', 'poly'], ['--lr_policy', 'poly', '-s', '40'], ['--lr_policy', 'cosine', '-s', '40'], ['-s', '40'], ['--lr_policy', 'exponential'],
                     ['--burn_in', '0'], ['--burn_in', '3'], ['--accum_steps', '0'], ['--weight_decay', '-1'], ['-lr', '0.01', '--burn_in', '3']):
            if keys in recipes[:2] + recipes[5:7] or not argv or argv[0] in ('--accum_steps', '-s') or '-o' in argv or '40' in argv:       # (every flag over four configs, the cross-key flags over all)
                train('recipe_setting', keys, argv)
    for keys in ({}, dict(accum_steps='4'), dict(weight_decay='0.0005')):
        for argv in ([], ['--accum_steps', '2'], ['--accum_steps', '1'], ['--weight_decay', '0.001']):
            train('recipe_setting', keys, argv, model='yolo')
    train('recipe_setting', dict(lr_policy='exponential'), [], decay=True)
    train('recipe_setting', {}, ['--lr_policy', 'exponential', '--burn_in', '3'], decay=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'option_cases.json.gz'))
    ap.add_argument('--commit', default=None, help='the commit whose answers these are (default: the checkout\'s HEAD)')
    args = ap.parse_args()
    commit = args.commit or subprocess.run(['git', '-C', ROOT, 'rev-parse', 'HEAD'], capture_output=True, text=True).stdout.strip() or 'unknown'
    rows = [json.dumps([fn, config, encode(a), outcome(fn, config, a)], separators=(',', ':')) for fn, config, a in cases()]
    text = '{\n "commit": %s,\n "cases": [\n%s\n ]\n}\n' % (json.dumps(commit), ',\n'.join('  ' + r for r in rows))       # one case per line: zcat shows them
    with open(args.out, 'wb') as f, gzip.GzipFile(filename='', mode='wb', fileobj=f, mtime=0) as z:       # (no name, no time: the same cases give the same bytes)
        z.write(text.encode())
    print('wrote %s: %d cases, %d of them refusals' % (args.out, len(rows), sum('"raises"' in r for r in rows)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
