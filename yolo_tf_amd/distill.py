"""The ``[distill]`` section of the config and the command line's flags for it: objectness-scaled distillation of a small YOLOv2 network from a large
one.  Host logic only -- nothing here imports torch or the library.

A row of KEYS is name, kind, default and meaning.  ``options`` resolves every key (an argument wins over the section, the section over the default)
and refuses what is out of range, naming the key; an absent section, an empty ``teacher`` and ``weight = 0`` all mean off (``enabled``).  ``head`` and
``refuse_pair`` describe the two heads and refuse a pair the kernel cannot compare; they look at builders' models only, so they run before any
device work."""
import collections
import math

import numpy as np

SECTION = 'distill'
CLASS_TERMS = ('mse', 'kl')
TEACHER_DTYPES = ('bf16', 'f32')
Key = collections.namedtuple('Key', 'name kind default meaning')
KEYS = collections.OrderedDict((row[0], Key(*row)) for row in (
    ('teacher', 'list', (), "the teacher's config files, as for -c (empty: off)"),
    ('teacher_ckpt', 'text', '', "checkpoint of the teacher, a .npz file or a TensorFlow prefix (empty: the latest in the teacher's logdir)"),
    ('teacher_ema', 'bool', False, "use the teacher's averaged weights"),
    ('teacher_dtype', 'choice', 'bf16', "compute dtype of the teacher's forward: bf16 or f32"),
    ('weight', 'float', 1.0, 'global weight of the distillation term, >= 0 (0: off)'),
    ('objectness', 'float', 1.0, 'weight of the objectness term, >= 0'),
    ('coords', 'float', 1.0, 'weight of the box term, >= 0'),
    ('prob', 'float', 1.0, 'weight of the class term, >= 0'),
    ('class_term', 'choice', 'mse', 'class term: mse (squared error of the two softmaxes) or kl (T^2 KL(teacher || student))'),
    ('temperature', 'float', 1.0, 'softmax temperature T of the class term, > 0'),
    ('scale_by_objectness', 'bool', True, "weight the box and class terms by the teacher's objectness"),
))
KERNEL_KEYS = ('weight', 'objectness', 'coords', 'prob', 'class_term', 'temperature', 'scale_by_objectness')      # the keyword arguments of ops.distill_partials
SCALARS = ('distill_objectness', 'distill_coords', 'distill_prob', 'distill')                                      # what fetch() gains, in this order
_BOOL = {'1': True, 'yes': True, 'true': True, 'on': True, '0': False, 'no': False, 'false': False, 'off': False}


def refusal(key, value, what):
    return ValueError('[%s] %s = %r: %s' % (SECTION, key, value, what))


def _raw(config, key, given):
    if given.get(key) is not None:
        return given[key]
    if config is not None and hasattr(config, 'has_option') and config.has_option(SECTION, key):
        return config.get(SECTION, key)
    return KEYS[key].default


def options(config=None, **given):
    """Every key of the section as a dict: ``given[key]`` where it is not None, else the key's text in ``config``, else its default.  Raises ValueError
    naming the key for a value that cannot be read or is out of range (``teacher_dtype = int8`` among them: an int8 teacher is out of scope)."""
    unknown = sorted(set(given) - set(KEYS))
    if unknown:
        raise ValueError('[%s] has no key %s (it has: %s)' % (SECTION, ', '.join(unknown), ', '.join(KEYS)))
    out = {}
    for key, row in KEYS.items():
        v = _raw(config, key, given)
        if row.kind == 'list':
            v = tuple(v.split()) if isinstance(v, str) else tuple(str(p) for p in v)
        elif row.kind == 'text':
            v = str(v).strip()
        elif row.kind == 'bool':
            if not isinstance(v, bool):
                if str(v).strip().lower() not in _BOOL:
                    raise refusal(key, v, 'true or false')
                v = _BOOL[str(v).strip().lower()]
        elif row.kind == 'float':
            try:
                f = float(v)
            except (TypeError, ValueError):
                raise refusal(key, v, 'a number')
            if key == 'temperature':
                if not (f > 0.0 and math.isfinite(f)):
                    raise refusal(key, v, 'the temperature is positive and finite')
            elif not (f >= 0.0 and math.isfinite(f)):
                raise refusal(key, v, 'a weight is >= 0 and finite')
            v = f
        else:
            v = str(v).strip().lower()
            if key == 'teacher_dtype' and v == 'int8':
                raise refusal(key, v, 'an int8 teacher is out of scope; the teacher runs in bf16 or f32')
            choices = CLASS_TERMS if key == 'class_term' else TEACHER_DTYPES
            if v not in choices:
                raise refusal(key, v, 'one of %s' % ', '.join(choices))
        out[key] = v
    return out


def enabled(opt):
    """Whether a run distils: a teacher is named and the global weight is not 0."""
    return bool(opt['teacher']) and opt['weight'] > 0


def kernel_options(opt):
    return {k: opt[k] for k in KERNEL_KEYS}


def add_flags(parser):
    """train.py's flags: --teacher CFG [CFG ...], --teacher_ckpt PATH and one flag per other key (default None: the section, or the key's default, decides)."""
    parser.add_argument('--teacher', nargs='+', default=None, help="[%s] teacher: %s" % (SECTION, KEYS['teacher'].meaning))
    parser.add_argument('--teacher_ckpt', default=None, help='[%s] teacher_ckpt: %s' % (SECTION, KEYS['teacher_ckpt'].meaning))
    parser.add_argument('--teacher_ema', default=None, action='store_true', help='[%s] teacher_ema: %s' % (SECTION, KEYS['teacher_ema'].meaning))
    parser.add_argument('--no_teacher_ema', dest='teacher_ema', action='store_false', help='turns [%s] teacher_ema off' % SECTION)
    parser.add_argument('--teacher_dtype', default=None, help='[%s] teacher_dtype: %s' % (SECTION, KEYS['teacher_dtype'].meaning))
    for key in ('weight', 'objectness', 'coords', 'prob', 'temperature'):
        parser.add_argument('--distill_' + key, default=None, type=float, help='[%s] %s: %s' % (SECTION, key, KEYS[key].meaning))
    parser.add_argument('--distill_class_term', default=None, choices=list(CLASS_TERMS), help='[%s] class_term: %s' % (SECTION, KEYS['class_term'].meaning))
    parser.add_argument('--distill_scale_by_objectness', default=None, action='store_true', help='[%s] scale_by_objectness: %s' % (SECTION, KEYS['scale_by_objectness'].meaning))
    parser.add_argument('--no_distill_scale_by_objectness', dest='distill_scale_by_objectness', action='store_false', help='turns [%s] scale_by_objectness off' % SECTION)


def from_args(args):
    """The flags of ``add_flags`` as the keyword arguments of ``options`` (None where a flag was not given)."""
    return {key: getattr(args, key if key.startswith('teacher') else 'distill_' + key, None) for key in KEYS}


def head(models, v1=False, batch=None, int8=False, name=''):
    """What ``refuse_pair`` compares, of one side: ``models`` maps (width, height) to the side's model at that input size."""
    m0 = next(iter(models.values()))
    anchors = None if v1 else np.asarray(m0.anchors, np.float32).reshape(-1, 2)
    return dict(name=name, v1=bool(v1), A=None if v1 else len(anchors), C=m0.classes, anchors=anchors, batch=batch, int8=bool(int8),
                grids={(int(w), int(h)): (m.cell_height, m.cell_width) for (w, h), m in models.items()})


def refuse_pair(student, teacher):
    """Raises for a pair of ``head`` dicts the distill kernel cannot compare, naming the cause: YOLO (v1) on either side, an int8 teacher, different anchor
    counts, class counts, anchors or grids at a size the student trains at (a size the teacher was not built with among them), a teacher batch
    smaller than the student's."""
    for side, h in (('student', student), ('teacher', teacher)):
        if h['v1']:
            raise NotImplementedError('distillation covers the YOLOv2 family: the %s is a YOLO (v1) network, whose fully connected head has no anchors to pair' % side)
    if teacher['int8']:
        raise NotImplementedError('distillation from an int8 teacher is out of scope: build the teacher session in bf16 or f32')
    if student['A'] != teacher['A']:
        raise ValueError('distillation pairs the lanes of two heads: the teacher has %d anchors, the student %d' % (teacher['A'], student['A']))
    if student['C'] != teacher['C']:
        raise ValueError('distillation pairs the lanes of two heads: the teacher has %d classes, the student %d' % (teacher['C'], student['C']))
    if not np.array_equal(student['anchors'], teacher['anchors']):
        raise ValueError('distillation compares w and h as logits, which needs shared anchors: the teacher\'s anchors differ from the student\'s')
    for wh, grid in sorted(student['grids'].items()):
        if wh not in teacher['grids']:
            raise ValueError('distillation: the student trains at %dx%d, a size the teacher session was not built with (build it with the same sizes)' % wh)
        if teacher['grids'][wh] != grid:
            raise ValueError('distillation pairs the cells of two heads: at %dx%d the teacher\'s grid is %dx%d, the student\'s %dx%d'
                             % (wh + tuple(teacher['grids'][wh][::-1]) + tuple(grid[::-1])))
    if student['batch'] is not None and teacher['batch'] is not None and teacher['batch'] < student['batch']:
        raise ValueError('distillation runs the teacher on the student\'s batch: the teacher session holds %d images, the student %d'
                         % (teacher['batch'], student['batch']))
