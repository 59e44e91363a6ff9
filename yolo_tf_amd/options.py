"""The ``[mi355x]`` section of the config: one table of every key the Python code reads, one reader, the command line's flags and their way into the config.

Host logic only -- nothing here imports torch or the library.  A NEW KEY IS ADDED HERE (a row of KEYS, and a ``;`` line in config.ini, which
tests/test_options_cpu.py asks for); the feature it belongs to reads it with ``read`` and keeps its own range checks and cross-key rules next to its code.
A row is name, kind, default (what ``read`` returns where the key is absent), meaning and, for the kind choice, the set.  The kinds: bool, int, float
(configparser's getboolean / getint / getfloat), choice and text (the text as it stands), ints and floats (a list of numbers separated by spaces or commas)."""
import collections

SECTION = 'mi355x'
Key = collections.namedtuple('Key', 'name kind default meaning choices')
KEYS = collections.OrderedDict((row[0], Key(*(row + (None,))[:5])) for row in (
    ('dtype', 'choice', 'bf16', 'compute dtype of activations and prepared filters (int8: detect.py / eval.py with a calibration)', ('bf16', 'f32', 'int8')),
    ('bucket_mb', 'float', 64.0, 'gradient all-reduce bucket size of data-parallel training, MiB'),
    ('grad_dtype', 'choice', 'f32', 'wire format of the gradient all-reduce', ('f32', 'bf16')),
    ('deterministic', 'bool', False, 'bitwise reproducible training steps'),
    ('comm_cus', 'int', 32, "CUs left to the collective's kernels in data-parallel runs (0: none)"),
    ('shard_optimizer', 'bool', False, 'data parallel: reduce-scatter, update 1/world, all-gather'),
    ('sync_bn', 'bool', False, 'batch normalisation statistics over all replicas'),
    ('multiscale', 'text', '', "input sizes a training run draws from: entries S, WxH or LO-HI (squares in steps of the network's stride) separated by spaces or commas (empty: one size)"),
    ('multiscale_every', 'int', 10, 'steps a drawn size holds, >= 1'),
    ('nms', 'choice', 'hard', "suppression of detect.py and eval.py: hard (the reference's NMS) or Soft-NMS with a linear or gaussian decay", ('hard', 'linear', 'gaussian')),
    ('nms_sigma', 'float', 0.5, 'nms gaussian: the decay is exp(-IoU^2 / sigma), at least 1/64'),
    ('tta', 'text', '', "test-time augmentation: the views, flip and / or sizes (S, WxH, LO-HI) separated by spaces or commas, e.g. 'flip 320 608', fused on the device into one result (empty: off; eval.py: not with --sizes)"),
    ('tta_iou', 'float', 0.55, "tta: a box joins a fused box at this IoU or above (the paper's default; not tuned here)"),
    ('mosaic', 'float', 0.0, 'probability that a training image is a 2x2 mosaic, in [0, 1]'),
    ('mosaic_scale', 'floats', (0.5, 1.5), "LO HI, 0 < LO <= HI: a tile's size relative to the frame"),
    ('mosaic_center', 'float', 0.25, 'the centre is drawn from [c, 1 - c] of the frame, c in [0, 0.5]'),
    ('mosaic_min_visible', 'float', 0.25, "share of a box's area that must stay visible, in [0, 1]"),
    ('mosaic_fill', 'float', 114.0, 'grey level where no tile reaches, in [0, 255]'),
    ('mixup', 'float', 0.0, 'probability that a training image is blended with a second one, in [0, 1]'),
    ('mixup_alpha', 'float', 1.5, 'lam ~ Beta(alpha, alpha), alpha > 0'),
    ('ema_decay', 'float', 0.0, 'decay of the weight average, in [0, 1) (0: off)'),
    ('box_loss', 'choice', 'mse', "box regression term of the YOLOv2 loss: mse (the reference's squared error) or 1 - IoU / GIoU / DIoU / CIoU of the responsible anchor's box", ('mse', 'iou', 'giou', 'diou', 'ciou')),
    ('class_loss', 'choice', 'mse', 'class term of the YOLOv2 loss: mse (squared error on the softmax), ce (cross-entropy) or focal', ('mse', 'ce', 'focal')),
    ('ignore_thresh', 'float', 0.0, 'IoU with a ground truth box above which a lane that is not responsible leaves the no-object term, inside (0, 1) (Darknet: 0.6; 0: off)'),
    ('rescore', 'bool', False, "the responsible anchor's objectness target is its IoU"),
    ('label_smoothing', 'float', 0.0, 'epsilon of the ce / focal class target, in [0, 1)'),
    ('focal_gamma', 'float', 2.0, 'focusing exponent of class_loss focal, 0 or >= 1'),
    ('accum_steps', 'int', 1, "micro-batches of one optimizer update (Darknet's subdivisions), >= 1 (1: off)"),
    ('weight_decay', 'float', 0.0, 'decay of the convolution and fully connected filters, >= 0 (Darknet: 0.0005; 0: off)'),
    ('weight_decay_mode', 'choice', 'l2', 'l2 (wd * w joins the gradient) or decoupled (AdamW: the filters are scaled by 1 - lr * wd ahead of the update)', ('l2', 'decoupled')),
    ('lr_policy', 'choice', None, 'learning-rate schedule (absent: [exponential_decay] when present, else constant)', ('exponential', 'constant', 'steps', 'poly', 'cosine')),
    ('lr_steps', 'ints', (), 'lr_policy steps: the updates at which the rate is scaled, ascending'),
    ('lr_scales', 'floats', (), 'lr_policy steps: one scale per entry of lr_steps'),
    ('lr_max_steps', 'int', 0, 'lr_policy poly / cosine: the update at which the schedule ends (train.py: -s)'),
    ('lr_power', 'float', 4.0, 'lr_policy poly: the exponent'),
    ('lr_min_ratio', 'float', 0.0, 'lr_policy cosine: the floor as a share of the rate, in [0, 1]'),
    ('burn_in', 'int', 0, 'the rate is multiplied by min(1, (step + 1) / N) ** burn_in_power over the first N updates (0: off)'),
    ('burn_in_power', 'float', 4.0, 'exponent of the burn-in ramp')))


def has(config, key):
    """Whether ``config`` sets ``key``: no for None, for a config without the section and for an object that is no config."""
    KEYS[key]          # (KeyError: a key the table does not hold)
    return config is not None and hasattr(config, 'has_option') and config.has_option(SECTION, key)


def refusal(config, key, what):
    """The ValueError that names the key, its text and ``what`` is wrong with it."""
    return ValueError('[%s] %s = %r: %s' % (SECTION, key, config.get(SECTION, key), what))


def read(config, key, given=None, how='kind', invalid=None):
    """The value of ``key``: ``given`` (an argument, the command line) if it is not None, else the key's text in ``config``, else its default.  ``how``
    the text is read: 'kind' -- as the key's kind; 'text' -- as it stands (for a caller whose refusal quotes it); 'list' -- an int or float key as a list of
    numbers too (the schedule and the composition accept ``4,`` for 4 and then ask for a list of one).  A text that cannot be read raises the
    ValueError of configparser (of int, float), or with ``invalid`` the ``refusal`` that says so."""
    if given is not None:
        return given
    if not has(config, key):
        return KEYS[key].default
    kind = KEYS[key].kind
    try:
        if how == 'list' or (how == 'kind' and kind in ('ints', 'floats')):
            number = int if kind in ('int', 'ints') else float
            return [number(v) for v in config.get(SECTION, key).replace(',', ' ').split()]
        getter = {'bool': config.getboolean, 'int': config.getint, 'float': config.getfloat}.get(kind, config.get) if how == 'kind' else config.get
        return getter(SECTION, key)
    except ValueError:
        if invalid is None:
            raise
        raise refusal(config, key, invalid)


def add_flags(parser, keys):
    """One ``--key`` per key for a command line (a pair is (flag, key) where the flag is spelled otherwise): type, choices and help from the table, default None."""
    for flag, key in (k if isinstance(k, tuple) else (k, k) for k in keys):
        k = KEYS[key]
        how = {'int': dict(type=int), 'float': dict(type=float), 'choice': dict(choices=list(k.choices or ())), 'ints': dict(nargs='+'), 'floats': dict(nargs='+')}.get(k.kind, {})
        parser.add_argument('--' + flag, default=None, help='overrides [%s] %s: %s' % (SECTION, key, k.meaning.replace('%', '%%')), **how)


def write(config, args, keys):
    """The command line over the config: every key of ``keys`` whose attribute of ``args`` is not None is written into the section (made if it is
    missing), a list as its entries separated by blanks, so that whatever reads the config afterwards finds it."""
    for key in keys:
        value = getattr(args, key)
        if value is not None:
            if not config.has_section(SECTION):
                config.add_section(SECTION)
            config.set(SECTION, key, ' '.join(str(v) for v in value) if isinstance(value, (list, tuple)) else str(value))
