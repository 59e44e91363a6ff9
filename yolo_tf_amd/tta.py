"""Test-time augmentation: the list of views one image is run at, before the device fuses their detections (csrc/tta.hip; Weighted Boxes
Fusion: Solovyev, Wang, Gabruseva 2021).

Host logic only -- nothing here imports torch.  A view is ``(width, height, flip)``; the first view of a list is the base view, whose grid is
the frame of the fused result.  ``parse_views`` reads the spec of ``--tta`` / ``[mi355x] tta``, ``describe`` is its text for logs and JSON,
``options`` reads the two config keys the way ``utils.nms_options`` reads its own."""
import re

from . import multiscale
from .options import KEYS as OPTION_KEYS, read as read_option

KEY, KEY_IOU = 'tta', 'tta_iou'
DEFAULT_IOU = OPTION_KEYS[KEY_IOU].default             # 0.55, the paper's default; not tuned here
M_LIMIT = 32768                # yolo2_wbf: pooled boxes per image


def parse_views(spec, base_wh, dw, dh):
    """``spec``: tokens separated by blanks or commas: ``flip`` and the size entries of ``multiscale.parse_sizes`` (``S``, ``WxH``, ``LO-HI``).
    -> [(width, height, flip)]: the base size without flip first, then every other size (by area, then width), then, if ``flip`` was
    given, the mirrored copy of each in the same order; duplicates are dropped.  ``flip`` alone gives two views; an empty spec gives []
    (off).  Anything else raises ValueError naming the token."""
    tokens = [t for t in re.split(r'[\s,]+', (spec or '').strip()) if t]
    if not tokens:
        return []
    flip = any(t.lower() == 'flip' for t in tokens)
    base = (int(base_wh[0]), int(base_wh[1]))
    sizes = [base]
    for t in tokens:
        if t.lower() == 'flip':
            continue
        try:
            found = multiscale.parse_sizes(t, dw, dh)
        except ValueError as e:
            raise ValueError('tta token %r: %s (a token is flip, S, WxH or LO-HI)' % (t, e))
        sizes += found
    rest = sorted(set(sizes) - {base}, key=lambda wh: (wh[0] * wh[1], wh[0]))
    views = [(w, h, False) for w, h in [base] + rest]
    if flip:
        views += [(w, h, True) for w, h, _ in views]
    return views


def view_sizes(views):
    """The distinct (width, height) of the views, the base size first."""
    out = []
    for w, h, _ in views:
        if (w, h) not in out:
            out.append((w, h))
    return out


def flip_only(views):
    return len(view_sizes(views)) == 1


def normalise(views):
    """[(width, height, flip)] with ints and bools; the first must not be flipped (it is the frame) and none may repeat."""
    views = [(int(w), int(h), bool(f)) for w, h, f in views]
    if not views:
        raise ValueError('tta: an empty view list (pass None to switch test-time augmentation off)')
    if views[0][2]:
        raise ValueError('tta: the first view is the base view and cannot be flipped')
    if len(set(views)) != len(views):
        raise ValueError('tta: a view is listed twice')
    return views


ROWS_BOUND = 65536


def evaluation_rows(M, C):
    """Rows of the fused buffers per image for an evaluation: a fused row is one (box, class) and the evaluation's threshold lets a box pass
    in several classes, so up to M * C rows can be needed; bounded by ROWS_BOUND (or M, if that is larger) to bound the [B,R,C] buffer.  An
    image that still overflows is reported (DetectSession.tta_check)."""
    return min(int(M) * int(C), max(int(M), ROWS_BOUND))


def describe(views):
    """``416 320 608 416+flip ...``: sizes as ``multiscale.describe`` writes them, ``+flip`` on the mirrored views."""
    return ' '.join(multiscale.describe([(w, h)]) + ('+flip' if f else '') for w, h, f in views)


def options(config, spec=None, iou=None):
    """(spec, fuse_iou): ``[mi355x] tta`` / ``tta_iou`` of ``config``, overridden by the arguments (the command line's) that are not None."""
    spec, iou = read_option(config, KEY, spec), float(read_option(config, KEY_IOU, iou))
    if not (iou == iou and abs(iou) != float('inf')):
        raise ValueError('[mi355x] %s = %r: the fusion overlap must be finite' % (KEY_IOU, iou))
    return spec, iou
