"""Multi-scale training and evaluation: the list of input sizes and the schedule that picks one per block of steps (YOLO9000, section 2:
"every 10 batches our network randomly chooses a new image dimension size ... multiples of 32: {320, 352, ..., 608}"; the reference lists
it as future work, README.md:87).

Host logic only -- nothing here imports torch.  ``parse_sizes`` reads the spec of ``[mi355x] multiscale`` / ``--multiscale`` / ``--sizes``,
``SizeSchedule`` is a pure function of the global step, ``configure`` turns a config (plus command-line overrides) into the size list of a
run or into None when the key is absent, and ``follow`` is the training loop's size handling: it binds the session to the step's size."""
import logging
import re

import numpy as np

from . import options

KEY, KEY_EVERY = 'multiscale', 'multiscale_every'
DEFAULT_EVERY = options.KEYS[KEY_EVERY].default              # 10, the paper's value


def parse_sizes(spec, dw, dh):
    """``spec``: entries separated by spaces or commas, each ``S`` (a square), ``WxH`` or ``LO-HI`` (squares from LO to HI inclusive in steps
    of ``dw``).  Every width must be a multiple of ``dw`` and every height one of ``dh`` (utils.get_downsampling), otherwise ValueError names
    the entry and the stride.  -> [(width, height)] without duplicates, sorted by (area, width); an empty spec gives []."""
    dw, dh = int(dw), int(dh)
    sizes = set()
    for entry in re.split(r'[\s,]+', (spec or '').strip()):
        if not entry:
            continue
        square, pair, span = re.match(r'^(\d+)$', entry), re.match(r'^(\d+)[xX](\d+)$', entry), re.match(r'^(\d+)-(\d+)$', entry)
        if square:
            found = [(int(square.group(1)),) * 2]
        elif pair:
            found = [(int(pair.group(1)), int(pair.group(2)))]
        elif span:
            lo, hi = int(span.group(1)), int(span.group(2))
            if lo > hi:
                raise ValueError('size entry %r: the range runs from %d down to %d' % (entry, lo, hi))
            if (hi - lo) % dw:
                raise ValueError('size entry %r: %d is not a whole number of steps of the stride %d above %d' % (entry, hi, dw, lo))
            found = [(s, s) for s in range(lo, hi + 1, dw)]
        else:
            raise ValueError('size entry %r is none of S, WxH and LO-HI' % entry)
        for w, h in found:
            if w <= 0 or w % dw:
                raise ValueError('size entry %r: the width %d is not a positive multiple of the stride %d' % (entry, w, dw))
            if h <= 0 or h % dh:
                raise ValueError('size entry %r: the height %d is not a positive multiple of the stride %d' % (entry, h, dh))
            sizes.add((w, h))
    return sorted(sizes, key=lambda wh: (wh[0] * wh[1], wh[0]))


class SizeSchedule(object):
    """``at(global_step)`` -> (width, height): one draw per block of ``every`` steps, a pure function of (seed, block).  The step that takes
    global_step from g to g + 1 runs at ``at(g)``.  There is no rank input: every data-parallel rank draws the same size without talking,
    and a run resumed from a checkpoint continues the schedule it left."""

    def __init__(self, sizes, every=DEFAULT_EVERY, seed=0):
        self.sizes = [(int(w), int(h)) for w, h in sizes]
        self.every, self.seed = int(every), int(seed)
        if not self.sizes:
            raise ValueError('a size schedule needs at least one size')
        if self.every < 1:
            raise ValueError('%s = %d: a size holds for at least one step' % (KEY_EVERY, self.every))

    def index_at(self, global_step):
        return int(np.random.RandomState((self.seed * 1000003 + int(global_step) // self.every) % 2 ** 32).randint(len(self.sizes)))

    def at(self, global_step):
        return self.sizes[self.index_at(global_step)]


def configure(config, spec=None, every=None):
    """The multi-scale setting of a run: ``[mi355x] multiscale`` / ``multiscale_every`` of ``config``, overridden by ``spec`` / ``every`` (the
    command line's) when those are not None.  -> None when the spec is absent or empty -- nothing about the run changes then -- otherwise
    (sizes, every, added): the sorted size list, which always holds the configured width x height (``added`` says whether it had to be put
    in).  Raises ValueError naming the key and the reason: the YOLO (v1) family, a bad entry, a list no member of which contains the rest."""
    from . import utils
    spec = options.read(config, KEY, spec)
    if not spec.strip():
        return None
    model = config.get('config', 'model')
    if model == 'yolo':
        raise ValueError('[mi355x] %s = %r: the fully connected head of the YOLO (v1) family fixes the input size' % (KEY, spec))
    every = options.read(config, KEY_EVERY, every)
    if int(every) < 1:
        raise ValueError('[mi355x] %s = %d: a size holds for at least one step' % (KEY_EVERY, every))
    dw, dh = utils.get_downsampling(config)
    try:
        sizes = parse_sizes(spec, dw, dh)
    except ValueError as e:
        raise ValueError('[mi355x] %s = %r: %s' % (KEY, spec, e))
    own = (config.getint(model, 'width'), config.getint(model, 'height'))
    added = own not in sizes
    if added:
        sizes = parse_sizes(' '.join('%dx%d' % wh for wh in sizes + [own]), dw, dh)
    check_nested(sizes, '[mi355x] %s = %r' % (KEY, spec))
    return sizes, int(every), added


def check_nested(sizes, what):
    """One set of buffers serves every size, allocated for the largest: that one must contain all the others."""
    w, h = max(sizes, key=lambda wh: wh[0] * wh[1])
    outside = [wh for wh in sizes if wh[0] > w or wh[1] > h]
    if outside:
        raise ValueError('%s: %s does not fit into the largest size %dx%d, for which the buffers are allocated'
                         % (what, ', '.join('%dx%d' % wh for wh in outside), w, h))


def describe(sizes):
    return ' '.join('%d' % w if w == h else '%dx%d' % (w, h) for w, h in sizes)


def follow(session, schedule, log=None):
    """The training loop's size handling, called before every step: binds ``session`` to ``schedule.at(session.global_step)`` and logs one
    line when that changes the size.  ``schedule`` None (no multi-scale): nothing happens.  -> the size the next step runs at."""
    if schedule is None:
        return session.size
    size = schedule.at(session.global_step)
    if size != session.size:
        (log or logging).warning('step %d: input size %dx%d' % (session.global_step, size[0], size[1]))
        session.set_size(*size)
    return size
