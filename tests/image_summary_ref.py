"""Specification of the image summaries (NumPy): TensorFlow 1.x ``core/kernels/summary_image_op.cc`` (``NormalizeFloatImage``) and the
reference's wrapper (train.py:44-53 there: channel counts other than 1, 3, 4 are summed to one channel), restated.

UNPINNED against TensorFlow: no TensorFlow is available to the tests, so this file is a careful restatement, not a recorded output of
``tf.summary.image``.  The kernel (csrc/image_summary.hip) has to equal it bitwise.

The rules, per image of a tensor [B, H, W, C] (f32, or bf16 widened exactly to f32; TF's own half-precision path is not reproduced):

1. C not in (1, 3, 4): the image becomes ONE channel, the sum over C.  ORDER OF THE SUM (this file's choice, the kernel follows it): the
   channels are cut into groups of GROUP = 8 consecutive channels (the last group may be short).  Inside a group the values are added in
   ascending channel order to an f64 partial that starts at +0.0; the partials are then added in ascending group order to an f64 total
   that starts at +0.0; the total is rounded once to f32.  depth = 1.  Otherwise depth = C and nothing is added.
2. The first min(image_max, B) images are taken; image_max < 1 is an error (TF's attribute max_images >= 1).
3. A pixel is finite when all its depth values are.  image_min / image_max are the minimum and maximum over all values of the finite
   pixels, +inf / -inf when there are none.  (The sign of a zero minimum or maximum is not specified: nothing below depends on it.)
4. image_min < 0:  m = max(|image_min|, |image_max|);  scale = 0 if m < float32(1e-6) else float32(127) / m;  offset = 128.
   otherwise:      scale = 0 if image_max < float32(1e-6) else float32(255) / image_max;  offset = 0.        (f32 divisions)
5. A finite pixel's bytes are uint8(trunc(x * scale + offset)): an f32 multiply, then an f32 add, each rounded (no fused multiply-add).
   A non-finite pixel becomes the bad colour (255, 0, 0, 255)[:depth].
6. Tag: ``<name>/image`` when the configured image_max is 1, otherwise ``<name>/image/<i>``.
7. Container: PNG, 8 bits, colour type 0 / 2 / 6 for depth 1 / 3 / 4, filter type 0 on every row (yolo_tf_amd/utils/png.py)."""
import numpy as np

GROUP = 8
BAD_COLOR = (255, 0, 0, 255)
ZERO_THRESHOLD = np.float32(1e-6)


def widen(x):
    """f32 view of the input: f32 as it is; a uint16 array is taken as bf16 bit patterns."""
    x = np.asarray(x)
    if x.dtype == np.uint16:
        return (x.astype(np.uint32) << 16).view(np.float32)
    assert x.dtype == np.float32, x.dtype
    return x


def channel_sum(x):
    """Rule 1 on [..., C] f32 -> [...] f32."""
    x = np.asarray(x, np.float32)
    c = x.shape[-1]
    total = np.zeros(x.shape[:-1], np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for g in range(0, c, GROUP):
            part = np.zeros(x.shape[:-1], np.float64)
            for j in range(g, min(g + GROUP, c)):
                part = part + x[..., j].astype(np.float64)
            total = total + part
        return total.astype(np.float32)


def depth_of(c):
    return c if c in (1, 3, 4) else 1


def normalize_image(img):
    """Rules 3-5 on one image [H, W, depth] f32 -> (uint8 [H, W, depth], {'min', 'max', 'scale', 'offset', 'nonfinite'})."""
    img = np.asarray(img, np.float32)
    assert img.ndim == 3 and img.shape[-1] in (1, 3, 4)
    finite = np.isfinite(img).all(axis=-1)
    vals = img[finite]
    image_min = np.float32(vals.min()) if vals.size else np.float32(np.inf)
    image_max = np.float32(vals.max()) if vals.size else np.float32(-np.inf)
    if image_min < 0:
        m = np.float32(max(abs(image_min), abs(image_max)))
        scale = np.float32(0) if m < ZERO_THRESHOLD else np.float32(127) / m
        offset = np.float32(128)
    else:
        scale = np.float32(0) if image_max < ZERO_THRESHOLD else np.float32(255) / image_max
        offset = np.float32(0)
    assert np.asarray(scale).dtype == np.float32
    out = np.empty(img.shape, np.uint8)
    out[...] = np.array(BAD_COLOR[:img.shape[-1]], np.uint8)
    with np.errstate(invalid='ignore', over='ignore'):
        prod = (vals * scale).astype(np.float32)           # rounded to f32 ...
        y = (prod + offset).astype(np.float32)             # ... before the add
    out[finite] = np.trunc(y).astype(np.uint8)
    return out, {'min': float(image_min), 'max': float(image_max), 'scale': float(scale), 'offset': float(offset), 'nonfinite': int((~finite).sum())}


def tags(name, image_max, batch):
    if image_max < 1:
        raise ValueError('image_max must be >= 1')
    n = min(image_max, batch)
    return [name + '/image'] if image_max == 1 else ['%s/image/%d' % (name, i) for i in range(n)]


def image_summary(name, x, image_max):
    """The whole summary of a tensor [B, H, W, C]: [(tag, uint8 [H, W, depth], info)]."""
    x = widen(x)
    assert x.ndim == 4
    names = tags(name, image_max, x.shape[0])
    if x.shape[-1] not in (1, 3, 4):
        x = channel_sum(x)[..., None]
    return [(tag,) + normalize_image(x[i]) for i, tag in enumerate(names)]
