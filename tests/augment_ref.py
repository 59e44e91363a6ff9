"""A float64 reference of the input pipeline (csrc/augment.hip), written from the definitions of the operations and sharing nothing with
oracle/yolo2_ref.py: NumPy only, no import from oracle/ or from the package.

The oracle restates the TF-1.0 kernels in f32 in their operation order, and so does the device kernel: what is wrong in that restatement is
wrong on both sides.  Here every operation is its textbook form in float64: bilinear interpolation as a * (1 - t) + b * t, HSV as in
`colorsys` with a PERIODIC hue (a hue of 1 is a hue of 0), contrast around the exact mean.  Scalar parameters are rounded to f32 first, since
the ABI carries them as f32; nothing else is.  What the two sides may differ by is therefore f32 rounding only (tests/augment_cases.py,
ORACLE_VS_F64_TOL).

Two conventions of the TF kernels that a textbook leaves open are taken over, and said here: the taps of the resize are floor and
min(floor + 1, size - 1) of out * (in / out) (no half-pixel centre), and saturation is 0 where v == 0.  For v < 0 (brightness can push a
whole pixel below zero) s = range / v is negative; the saturation op clips it to 0, which is what the TF kernel's `v > 0` guard gives as
well.  A hue rotation alone of such a pixel is the one place where this definition and TF's differ (TF returns grey); no case does that.
"""
import numpy as np

f32 = lambda v: float(np.float32(v))


def crop(img, box):
    """box = (x0, y0, w, h) or None."""
    if box is None:
        return img
    x0, y0, w, h = box
    return img[y0:y0 + h, x0:x0 + w]


def taps(in_size, out_size):
    """(lower tap, upper tap, weight of the upper tap) of every output position along one axis."""
    pos = np.arange(out_size, dtype=np.float64) * (float(in_size) / float(out_size))
    lo = np.floor(pos).astype(np.int64)
    hi = np.minimum(lo + 1, in_size - 1)
    return lo, hi, pos - lo


def resize(img, out_h, out_w):
    img = np.asarray(img, np.float64)
    in_h, in_w = img.shape[:2]
    if (in_h, in_w) == (out_h, out_w):
        return img
    ylo, yhi, ty = taps(in_h, out_h)
    xlo, xhi, tx = taps(in_w, out_w)
    tx = tx[None, :, None]
    ty = ty[:, None, None]
    rows_lo, rows_hi = img[ylo], img[yhi]
    top = rows_lo[:, xlo] * (1 - tx) + rows_lo[:, xhi] * tx
    bottom = rows_hi[:, xlo] * (1 - tx) + rows_hi[:, xhi] * tx
    return top * (1 - ty) + bottom * ty


def to_hsv(rgb):
    rgb = np.asarray(rgb, np.float64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    v = rgb.max(-1)
    span = v - rgb.min(-1)
    safe = np.where(span == 0, 1.0, span)
    sector = np.stack([(g - b) / safe, 2 + (b - r) / safe, 4 + (r - g) / safe], -1)
    which = rgb.argmax(-1)
    h = np.mod(np.take_along_axis(sector, which[..., None], -1)[..., 0] / 6, 1.0)
    h = np.where(span == 0, 0.0, h)
    s = np.where(v == 0, 0.0, span / np.where(v == 0, 1.0, v))
    return h, s, v


def from_hsv(h, s, v):
    def f(n):
        k = np.mod(n + 6 * h, 6.0)
        return v - v * s * np.clip(np.minimum(k, 4 - k), 0, 1)
    return np.stack([f(5), f(3), f(1)], -1)


def saturation(img, factor):
    h, s, v = to_hsv(img)
    return from_hsv(h, np.clip(s * f32(factor), 0, 1), v)


def hue(img, delta):
    h, s, v = to_hsv(img)
    return from_hsv(np.mod(h + (1 + f32(delta)), 1.0), s, v)


def contrast(img, factor):
    mean = img.mean((0, 1), keepdims=True)
    return (img - mean) * f32(factor) + mean


def grey(img):
    g = img[..., 0] * 0.2989 + img[..., 1] * 0.5870 + img[..., 2] * 0.1140
    return np.repeat(g[..., None], 3, -1)


def augment_image(src_u8, p, width, height):
    """The chain of the device kernel for one image; `p` as for the oracle's augment_image: crop (x0, y0, w, h) or None, flip, brightness /
    saturation / hue / contrast (None: not taken), noise (None or an [H, W, 3] array already scaled), gray.  float64 [height, width, 3]."""
    img = resize(crop(np.asarray(src_u8, np.float64), p.get('crop')), height, width)
    if p.get('flip'):
        img = img[:, ::-1]
    if p.get('brightness') is not None:
        img = img + f32(p['brightness'])
    if p.get('saturation') is not None:
        img = saturation(img, p['saturation'])
    if p.get('hue') is not None:
        img = hue(img, p['hue'])
    if p.get('contrast') is not None:
        img = contrast(img, p['contrast'])
    if p.get('noise') is not None:
        img = img + np.asarray(p['noise'], np.float64)
    if p.get('gray'):
        img = grey(img)
    return np.clip(img, 0, 255)


def transform_labels(objects_class, objects_coord, classes, cell_width, cell_height):
    """Boxes (xmin, ymin, xmax, ymax) normalised to [0, 1] -> (mask [cells], prob [cells, classes], coords [cells, 4], offset_xy_min
    [cells, 2], offset_xy_max [cells, 2], areas [cells], error bits), float64, one object after the other.

    The responsible cell is the one the box centre falls into, addressed by the FLAT index iy * cell_width + ix, and only that flat index is
    range-checked: a centre at x == 1.0 exactly has ix == cell_width, which with iy < cell_height - 1 is a valid flat index, that of the first
    cell of the NEXT row.  The reference this project follows does exactly that and raises nothing, so this function does too, on purpose.
    Only an index outside [0, cells) or a class outside [0, classes) sets error bit 0 and skips the object; a negative extent of a written
    cell sets error bit 1.  Later objects overwrite the numbers of a shared cell; the class bits accumulate."""
    cells = cell_width * cell_height
    mask = np.zeros(cells)
    prob = np.zeros((cells, classes))
    coords = np.zeros((cells, 4))
    lo = np.zeros((cells, 2))
    hi = np.zeros((cells, 2))
    err = 0
    box = np.asarray(objects_coord, np.float64).reshape(-1, 4)
    for c, (xmin, ymin, xmax, ymax) in zip(np.asarray(objects_class).reshape(-1), box):
        x, y = cell_width * (xmin + xmax) / 2, cell_height * (ymin + ymax) / 2
        ix, iy = np.floor(x), np.floor(y)
        index = int(iy * cell_width + ix)
        if not (0 <= index < cells and 0 <= int(c) < classes):
            err |= 1
            continue
        w, h = xmax - xmin, ymax - ymin
        mask[index] = 1
        prob[index, int(c)] = 1
        with np.errstate(invalid='ignore'):
            coords[index] = (x - ix, y - iy, np.sqrt(w), np.sqrt(h))
        half = np.array([w / 2 * cell_width, h / 2 * cell_height])
        lo[index] = coords[index, :2] - half
        hi[index] = coords[index, :2] + half
    extent = hi - lo
    if (extent < 0).any():
        err |= 2
    return mask, prob, coords, lo, hi, extent[:, 0] * extent[:, 1], err
