"""The cases of the input pipeline kernels (csrc/augment.hip: yolo2_augment_images, yolo2_transform_labels), shared by
tests/test_augment_cases_cpu.py (no GPU: validates the table and measures the tolerance) and tests/test_augment_cases_gpu.py (launches the
kernels on them).  Seeded generators and literals only, no files; every case and every result is built once, cached and read-only.

An image case is one source image, one set of parameters and one output size; its id says what it pins.  `case(name)` gives
{'name', 'src' uint8 [h, w, 3], 'W', 'H', 'p', 'tags'} with `p` in the convention of oracle.yolo2_ref.augment_image and of
test_augment_gpu.run_augment (crop (x0, y0, w, h), flip, gray, brightness / saturation / hue / contrast, noise_scale / noise_seed).  The
`tags` name the property that tests/test_augment_cases_cpu.py proves the case to have (a tap beyond the crop, a hue of exactly 1.0f, ...).
Two references: `oracle(name)`, the f32 restatement the kernel is held to at 2e-3, and `f64(name)`, tests/augment_ref.py, which shares no
code with either.  A batch case is a list of such images packed into one source buffer (BATCHES); a label case is a list of images'
objects on one grid (LABELS).

Sources are at most 200 px on a side and outputs at most 150 px, with two exceptions that the sizes themselves force: H * W = 257 is
prime (257 x 1) and 32769 = 99 x 331 (the smallest factor pair), both still far below a second."""
import functools

import numpy as np

import augment_ref as F
from oracle import yolo2_ref as R

GPU_VS_ORACLE_TOL = 2e-3          # tests/test_augment_gpu.py::test_augment_images_matches_oracle, on the 0..255 scale
# Oracle (f32, TF operation order) against the float64 reference: the largest deviation, in grey levels, over every pixel of every image
# case and every image of every batch case of this file.  Measured with
#     python -m pytest tests/test_augment_cases_cpu.py -k measured_over -s        (prints the figure; the test fails once this
# constant is more than twice what it measures).  The tolerance is twice that: the factor covers the spread between seeds of a maximum over a few
# hundred thousand pixels.  Its source is f32 rounding: the sample position times the local gradient (size * 2^-24 * 255 * scale), and
# near a grey pixel the hue, whose error (2^-24 * 255 / range) a saturation or hue change turns into a channel.
ORACLE_VS_F64_MEASURED = 2.78e-3         # 2.7703e-03 at geom_hw32769 (331 rows from 190: the f32 row position times a gradient of up to 255), 176653 pixels
ORACLE_VS_F64_TOL = 2 * ORACLE_VS_F64_MEASURED

IMAGES = {}        # name -> (source spec, W, H, p, tags)


def _add(name, src, W, H, tags=(), **p):
    assert name not in IMAGES
    IMAGES[name] = (src, W, H, p, frozenset(tags))


# ---- resize geometry: (crop_w, crop_h) -> (W, H), once over a whole source and once over a crop with margin on every side
GEOMETRY = {
    'up2': (37, 23, 74, 46), 'up3p7': (30, 20, 111, 74), 'down2': (100, 60, 50, 30), 'down2p6': (131, 97, 50, 37),
    'tall_to_wide': (9, 150, 120, 8), 'wide_to_tall': (120, 8, 9, 150), 'w1': (40, 30, 1, 17), 'h1': (40, 30, 23, 1), 'copy': (45, 31, 45, 31),
    # a ragged last wave / a second trip of the grid-stride loop (128 blocks x 256 threads = 32768)
    'hw1': (12, 10, 1, 1), 'hw63': (20, 15, 7, 9), 'hw65': (5, 4, 13, 5), 'hw257': (100, 3, 257, 1), 'hw32769': (120, 190, 99, 331),
}
for _i, (_g, (_cw, _ch, _W, _H)) in enumerate(GEOMETRY.items()):
    _t = {'copy': ('copy',), 'down2': ('int_down',)}.get(_g, ())
    _add('geom_%s' % _g, ('rand', _ch, _cw, 100 + _i), _W, _H, _t)
    _add('geom_%s_cropped' % _g, ('rand', _ch + 5, _cw + 7, 200 + _i), _W, _H, _t, crop=(3, 2, _cw, _ch))

# ---- crop edge clamp: 0 inside the crop, 255 outside, upscaled: the last tap is floor + 1 = crop size, and must clamp to crop size - 1.
# A clamp at the source's edge reads 255 there.  The expected output is 0 everywhere.
for _name, _crop, _W, _H in (('interior', (2, 3, 11, 9), 29, 22), ('flush_right', (9, 3, 11, 9), 29, 22), ('flush_bottom', (2, 7, 11, 9), 29, 22),
                             ('flush_both', (9, 7, 11, 9), 29, 22), ('crop_w1', (5, 3, 1, 9), 6, 22), ('crop_h1', (2, 6, 11, 1), 29, 5),
                             ('last_pixel', (19, 15, 1, 1), 5, 4)):
    _add('clamp_%s' % _name, ('clamp', 16, 20, _crop), _W, _H, ('clamp',), crop=_crop)

# ---- flip
_add('flip_odd_w', ('rand', 20, 30, 301), 45, 31, flip=True)
_add('flip_w1', ('rand', 20, 30, 302), 1, 11, flip=True)
_add('flip_copy_cropped', ('rand', 36, 52, 303), 45, 31, ('copy',), crop=(3, 2, 45, 31), flip=True)
_add('flip_copy', ('rand', 31, 45, 304), 45, 31, ('copy',), flip=True)
_add('flip_down2', ('rand', 60, 100, 305), 50, 30, ('int_down',), flip=True)
_add('flip_down2_cropped', ('rand', 65, 107, 306), 50, 30, ('int_down',), crop=(3, 2, 100, 60), flip=True)

# ---- colour paths, each alone, at an upscale (block 2, 30 x 18 -> 67 x 41) and at a downscale (block 6, 90 x 66 -> 41 x 29)
for _d, _blk, _w, _h, _W, _H in (('up', 2, 30, 18, 67, 41), ('down', 6, 90, 66, 41, 29)):
    _s = 400 if _d == 'up' else 500
    _add('black_grey_saturation_%s' % _d, ('black_grey', _h, _w, _blk, _s + 1), _W, _H, ('v0',), saturation=1.3)
    _add('black_grey_hue_%s' % _d, ('black_grey', _h, _w, _blk, _s + 2), _W, _H, ('v0',), hue=0.02)
    _add('below0_saturation_%s' % _d, ('rand', _h, _w, _s + 3), _W, _H, ('below0',), brightness=-60.0, saturation=1.4)
    _add('above255_saturation_%s' % _d, ('rand', _h, _w, _s + 4), _W, _H, ('above255',), brightness=62.0, saturation=0.6)
    _add('saturation_clips_at_1_%s' % _d, ('vivid', _h, _w, _s + 5), _W, _H, ('satclip',), saturation=1.5)
    _add('hue_wrap_up_%s' % _d, ('near_red', _h, _w, _s + 6), _W, _H, ('wrap',), hue=0.032)
    _add('hue_wrap_down_%s' % _d, ('near_red', _h, _w, _s + 7), _W, _H, ('wrap',), hue=-0.032)
    _add('sectors_saturation_%s' % _d, ('sectors', _h, _w, _blk), _W, _H, ('sectors',), saturation=0.7)
    _add('sectors_hue_%s' % _d, ('sectors', _h, _w, _blk), _W, _H, ('sectors',), hue=0.02)
    _add('contrast_0p5_%s' % _d, ('rand', _h, _w, _s + 8), _W, _H, ('mean',), contrast=0.5)
    _add('contrast_1p5_%s' % _d, ('rand', _h, _w, _s + 9), _W, _H, ('mean', 'clip'), contrast=1.5)
    _add('grey_after_noise_%s' % _d, ('rand', _h, _w, _s + 10), _W, _H, ('grey',), noise_scale=15.0, noise_seed=77 + _blk, gray=True)

# ---- a hue of exactly 1.0f out of uint8 input: rgb_to_hsv wraps a tiny negative hue with h + 1, which rounds to 1.0f; a literal HSVToRGB
# switch then returns (m, m, m).  Two equal rows of r everywhere and (g, b) per column, resized in x only.  The first is the reproducer of
# the defect's report; the others were found by `search_hue1` (tests/test_augment_cases_cpu.py runs the search again and compares).
HUE1 = {
    'a': (169, 32, 28, (114, 126, 127, 19, 21, 130, 90, 82, 18, 107, 20, 81, 61, 88, 8, 41, 38, 85, 42, 108, 15, 67, 139, 64, 11, 116, 108, 2, 61,
                        84, 29, 131),
          (115, 127, 127, 19, 21, 130, 90, 82, 19, 108, 20, 82, 61, 89, 9, 42, 39, 85, 43, 109, 15, 67, 140, 64, 11, 117, 109, 2, 62, 84, 29, 132)),
    'b': (176, 56, 52, (99, 9, 47, 4, 75, 104, 26, 9, 89, 73, 28, 89, 109, 68, 30, 47, 33, 117, 93, 93, 84, 53, 80, 95, 38, 65, 65, 109, 30, 41, 116,
                        37, 42, 1, 62, 5, 14, 9, 85, 67, 30, 23, 81, 10, 47, 55, 48, 6, 70, 21, 35, 107, 27, 16, 38, 36),
          (100, 9, 48, 4, 76, 104, 27, 10, 90, 73, 28, 90, 110, 69, 30, 47, 34, 118, 93, 93, 85, 54, 80, 96, 38, 66, 66, 109, 30, 42, 116, 37, 42, 2, 62,
           6, 15, 10, 86, 67, 30, 24, 81, 10, 48, 55, 48, 6, 70, 21, 35, 107, 28, 16, 38, 36)),
    'c': (168, 60, 46, (27, 89, 116, 67, 47, 51, 24, 16, 25, 108, 97, 52, 35, 19, 2, 76, 114, 62, 33, 56, 12, 72, 59, 86, 61, 111, 112, 73, 40, 28, 89,
                        30, 38, 67, 74, 9, 63, 115, 29, 111, 4, 34, 61, 110, 103, 39, 34, 112, 8, 87, 43, 90, 45, 59, 2, 39, 30, 65, 21, 74),
          (28, 90, 116, 68, 48, 52, 24, 17, 25, 108, 97, 53, 35, 19, 2, 76, 115, 63, 33, 57, 12, 73, 59, 87, 62, 112, 112, 73, 40, 29, 89, 31, 38, 67, 75,
           10, 63, 116, 30, 111, 5, 34, 62, 110, 103, 40, 34, 113, 8, 87, 43, 90, 45, 60, 3, 40, 30, 65, 22, 75)),
    'd': (140, 33, 55, (21, 78, 114, 114, 47, 76, 1, 100, 54, 75, 27, 37, 101, 75, 60, 42, 62, 46, 65, 100, 0, 67, 105, 94, 99, 55, 92, 74, 65, 34, 61,
                        22, 62),          # an upscale
          (22, 78, 115, 114, 48, 76, 2, 101, 54, 75, 27, 38, 102, 76, 60, 42, 63, 46, 65, 100, 0, 68, 106, 95, 99, 55, 92, 74, 66, 35, 61, 23, 62)),
}
HUE1_SEARCH = dict(seed=0, draws=3000, want=3)
for _k in HUE1:
    _r, _in, _out, _, _ = HUE1[_k]
    _add('hue1_%s_saturation' % _k, ('hue1', _k), _out, 2, ('hue1',), saturation=1.3)
_add('hue1_a_brightness_saturation', ('hue1', 'a'), 28, 2, ('hue1',), brightness=-8.0, saturation=1.3)      # 11.0002 - 8 is exact in f32


def search_hue1(seed, draws, want=2):
    """At most `draws` seeded sources under 64 px, of the reproducer's kind (b - g is 0 or 1 per column); returns the first `want` whose
    resize holds a pixel of hue exactly 1.0f, with r and the size pair different from the reproducer's and from one another."""
    rng = np.random.RandomState(seed)
    found, used_r, used_sizes = [], {HUE1['a'][0]}, {HUE1['a'][1:3]}
    for _ in range(draws):
        w_in, w_out, r = int(rng.randint(8, 64)), int(rng.randint(8, 64)), int(rng.randint(120, 256))
        g = rng.randint(0, 118, w_in)
        b = g + rng.randint(0, 2, w_in)
        if w_in == w_out or r in used_r or (w_in, w_out) in used_sizes:
            continue
        hue = R.rgb_to_hsv(R.resize_bilinear(_hue1_source(r, g, b).astype(np.float32), 2, w_out))[..., 0]
        if (hue == np.float32(1)).any():
            found.append((r, w_in, w_out, tuple(int(v) for v in g), tuple(int(v) for v in b)))
            used_r.add(r)
            used_sizes.add((w_in, w_out))
            if len(found) == want:
                break
    return found


def _hue1_source(r, g, b):
    row = np.stack([np.full(len(g), r), np.asarray(g), np.asarray(b)], -1).astype(np.uint8)
    return np.stack([row, row])


# ---------------------------------------------------------------------------------------------------------------------
# sources
# ---------------------------------------------------------------------------------------------------------------------
PALETTE = ((255, 0, 0), (255, 255, 0), (0, 255, 0), (0, 255, 255), (0, 0, 255), (255, 0, 255),        # primaries and secondaries
           (200, 200, 90), (90, 200, 200), (200, 90, 200),                                          # two equal maxima, not saturated
           (220, 120, 30), (120, 220, 30), (30, 220, 120), (30, 120, 220), (120, 30, 220), (220, 30, 120))      # the inside of each sector


def _source(spec):
    kind = spec[0]
    if kind == 'rand':
        _, h, w, seed = spec
        return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == 'clamp':
        _, h, w, (x0, y0, cw, ch) = spec
        img = np.full((h, w, 3), 255, np.uint8)
        img[y0:y0 + ch, x0:x0 + cw] = 0
        return img
    if kind == 'black_grey':             # blocks of black (v == 0), of greys (range == 0 at v > 0) and of random colours
        _, h, w, blk, seed = spec
        rng = np.random.RandomState(seed)
        by, bx = -(-h // (2 * blk)), -(-w // (2 * blk))
        what = rng.randint(0, 3, (by, bx))
        grey = rng.randint(1, 256, (by, bx, 1)).repeat(3, -1)
        colour = rng.randint(0, 256, (by, bx, 3))
        blocks = np.where(what[..., None] == 0, 0, np.where(what[..., None] == 1, grey, colour))
        return blocks.repeat(2 * blk, 0).repeat(2 * blk, 1)[:h, :w].astype(np.uint8)
    if kind == 'vivid':                  # half of the pixels with a saturation of 0.75 .. 1 before the change
        _, h, w, seed = spec
        rng = np.random.RandomState(seed)
        img = rng.randint(0, 256, (h, w, 3))
        vivid = rng.rand(h, w) < 0.5                                   # the others stay as drawn: some products stay below 1
        img[..., 0] = np.where(vivid, np.maximum(img[..., 0], 160), img[..., 0])
        img[..., 2] = np.where(vivid, img[..., 2] % 40, img[..., 2])
        return img.astype(np.uint8)
    if kind == 'near_red':               # hue = +- d / 960, d in [0, 30]: within 0.032 of 0 and of 1
        _, h, w, seed = spec
        rng = np.random.RandomState(seed)
        d = rng.randint(0, 31, (h, w))
        above = rng.rand(h, w) < 0.5
        return np.stack([np.full((h, w), 200), 40 + np.where(above, d, 0), 40 + np.where(above, 0, d)], -1).astype(np.uint8)
    if kind == 'sectors':
        _, h, w, blk = spec
        assert w == blk * len(PALETTE)
        return np.tile(np.array(PALETTE, np.uint8).repeat(blk, 0)[None], (h, 1, 1))
    if kind == 'hue1':
        r, w_in, _, g, b = HUE1[spec[1]]
        assert len(g) == len(b) == w_in
        return _hue1_source(r, g, b)
    raise KeyError(kind)


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


NAMES = tuple(IMAGES)


@functools.lru_cache(maxsize=None)
def case(name):
    spec, W, H, p, tags = IMAGES[name]
    src = _frozen(_source(spec))
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 3
    if p.get('crop') is not None:
        x0, y0, w, h = p['crop']
        assert 0 <= x0 and 0 <= y0 and w >= 1 and h >= 1 and x0 + w <= src.shape[1] and y0 + h <= src.shape[0]      # the kernel trusts the crop
    return {'name': name, 'src': src, 'W': W, 'H': H, 'p': dict(p), 'tags': tags}


def host_noise(seed, scale, H, W):
    """A stand-in for the device's noise where no device is there: standard normals cut to |z| <= 2, times the f32 scale."""
    z = np.clip(np.random.RandomState(seed % (2 ** 31)).standard_normal((H, W, 3)), -2, 2)
    return _frozen((z * np.float32(scale)).astype(np.float32))


def with_noise(c, noise=None):
    """The case's parameters for a reference: `noise` as an array (the device's own, or host_noise where the case asks for noise)."""
    p = dict(c['p'])
    if p.get('noise_scale') is not None:
        p['noise'] = host_noise(p['noise_seed'], p['noise_scale'], c['H'], c['W']) if noise is None else noise
    return p


def oracle_of(c, noise=None):
    return _frozen(R.augment_image(c['src'], with_noise(c, noise), c['W'], c['H']))


def f64_of(c, noise=None):
    return _frozen(F.augment_image(c['src'], with_noise(c, noise), c['W'], c['H']))


@functools.lru_cache(maxsize=None)
def oracle(name):
    return oracle_of(case(name))


@functools.lru_cache(maxsize=None)
def f64(name):
    return f64_of(case(name))


def before_hsv(c):
    """The oracle's image as the HSV code first sees it: after crop, resize, flip and brightness."""
    p = {k: v for k, v in c['p'].items() if k in ('crop', 'flip', 'brightness')}
    img = np.asarray(c['src'], np.float32)
    if p.get('crop') is not None:
        x0, y0, w, h = p['crop']
        img = img[y0:y0 + h, x0:x0 + w]
    img = R.resize_bilinear(img, c['H'], c['W'])
    if p.get('flip'):
        img = img[:, ::-1]
    if p.get('brightness') is not None:
        img = img + np.float32(p['brightness'])
    return img


def exact_expectation(c):
    """For the copy-shortcut and integer-downscale cases: the source bytes the output must equal, bit for bit."""
    x0, y0, w, h = c['p'].get('crop') or (0, 0, c['src'].shape[1], c['src'].shape[0])
    img = c['src'][y0:y0 + h, x0:x0 + w]
    if 'int_down' in c['tags']:
        assert h == 2 * c['H'] and w == 2 * c['W']
        img = img[::2, ::2]
    assert img.shape[:2] == (c['H'], c['W'])
    return (img[:, ::-1] if c['p'].get('flip') else img).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# batches: name -> {'W', 'H', 'sources': [uint8 images, packed back to back in this order], 'items': [(source index, p)]}
# ---------------------------------------------------------------------------------------------------------------------
_COLOUR = (dict(), dict(flip=True), dict(brightness=-30.0), dict(saturation=1.4), dict(hue=-0.03), dict(gray=True),
           dict(brightness=25.0, saturation=0.6, hue=0.01), dict(flip=True, saturation=1.2, gray=True))


def _varied(rng, sources, n):
    items = []
    for i in range(n):
        k = i % len(sources)
        h, w = sources[k].shape[:2]
        p = dict(_COLOUR[i % len(_COLOUR)])
        if i % 3:
            cw, ch = int(rng.randint(1, w + 1)), int(rng.randint(1, h + 1))
            p['crop'] = (int(rng.randint(0, w - cw + 1)), int(rng.randint(0, h - ch + 1)), cw, ch)
        items.append((k, p))
    return items


def _batch(name):
    rng = np.random.RandomState({'b8': 8, 'b64': 64, 'b5_contrast_on_1_and_3': 5, 'shared_source': 6}.get(name, 3))
    rand = lambda h, w: rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if name in ('b8', 'b64'):                                            # the launcher's other two grids: 32 and 8 blocks per image
        sources = [rand(9 + 5 * i, 40 - 3 * i) for i in range(8)]
        return dict(W=7, H=5, sources=sources, items=_varied(rng, sources, int(name[1:])))
    if name == 'b5_contrast_on_1_and_3':                                 # pass A returns early for images 0, 2, 4: they must not touch the sums
        sources = [rand(20 + 7 * i, 50 - 6 * i) for i in range(5)]
        items = [(i, dict(_COLOUR[i + 1], **({'contrast': 0.5 + 0.4 * i} if i in (1, 3) else {}))) for i in range(5)]
        return dict(W=33, H=21, sources=sources, items=items)
    if name == 'shared_source':                                          # one offset, six crops
        sources = [rand(50, 60)]
        crops = ((0, 0, 60, 50), (7, 5, 31, 23), (59, 49, 1, 1), (0, 27, 60, 23), (29, 0, 31, 50), (10, 10, 20, 40))
        return dict(W=31, H=23, sources=sources, items=[(0, dict(_COLOUR[i], crop=c)) for i, c in enumerate(crops)])
    if name.startswith('packed_'):                                       # image A of three sizes first, in the middle and last
        a, b, c = rand(23, 31), rand(40, 17), rand(11, 64)
        order = {'packed_first': (a, b, c), 'packed_middle': (b, a, c), 'packed_last': (b, c, a)}[name]
        ps = {id(a): dict(saturation=1.3), id(b): dict(flip=True), id(c): dict(hue=0.02, crop=(5, 2, 40, 8))}
        return dict(W=29, H=19, sources=list(order), items=[(i, ps[id(s)]) for i, s in enumerate(order)])
    raise KeyError(name)


BATCHES = ('b8', 'b64', 'b5_contrast_on_1_and_3', 'shared_source', 'packed_first', 'packed_middle', 'packed_last')


@functools.lru_cache(maxsize=None)
def batch(name):
    b = _batch(name)
    b['sources'] = [_frozen(s) for s in b['sources']]
    b['offsets'] = [int(v) for v in np.cumsum([0] + [s.size for s in b['sources']])[:-1]]
    b['name'] = name
    return b


def batch_image(name, i):
    """Image i of a batch as an image case of its own."""
    b = batch(name)
    k, p = b['items'][i]
    return {'name': '%s[%d]' % (name, i), 'src': b['sources'][k], 'W': b['W'], 'H': b['H'], 'p': dict(p), 'tags': frozenset()}


def every_image():
    """Every image the tolerance is measured over: the image cases and the images of the batch cases."""
    for name in NAMES:
        yield case(name)
    for name in BATCHES:
        for i in range(len(batch(name)['items'])):
            yield batch_image(name, i)


# ---------------------------------------------------------------------------------------------------------------------
# labels: name -> (classes, cell_width, cell_height, [(classes [K], boxes [K, 4] f32 normalised) per image], error bits expected)
# ---------------------------------------------------------------------------------------------------------------------
def _objects(rng, k, classes):
    centre = rng.uniform(0.02, 0.98, (k, 2))
    size = rng.uniform(0.01, 0.6, (k, 2))
    box = np.clip(np.concatenate([centre - size / 2, centre + size / 2], 1), 0, 1).astype(np.float32)
    return rng.randint(0, classes, k).astype(np.int32), box


def _labels(name):
    rng = np.random.RandomState(sum(name.encode()))
    one = lambda cls, boxes: (np.asarray(cls, np.int32), np.asarray(boxes, np.float32).reshape(-1, 4))
    if name == 'grid_1x1':
        return 1, 1, 1, [_objects(rng, 3, 1), _objects(rng, 1, 1)], 0
    if name == 'grid_19x19_c80':                                         # the 608 px multi-scale size
        return 80, 19, 19, [_objects(rng, k, 80) for k in (9, 1, 30)], 0
    if name == 'grid_7x20':
        return 1, 7, 20, [_objects(rng, k, 1) for k in (6, 14)], 0
    if name == 'grid_20x7':
        return 1, 20, 7, [_objects(rng, k, 1) for k in (6, 14)], 0
    if name == 'centre_on_cell_boundary':                                # x * cw = 5 exactly: the cell to the right; y * ch = 0
        return 3, 20, 7, [one([2, 1], [[0.125, 0.25, 0.375, 0.5], [0.0, 0.0, 0.5, 0.0]])], 0
    if name == 'zero_extent':                                            # xmax == xmin, ymax == ymin: sqrt(0), area 0
        return 3, 13, 13, [one([0, 1, 2], [[0.3, 0.2, 0.3, 0.6], [0.1, 0.7, 0.5, 0.7], [0.9, 0.9, 0.9, 0.9]])], 0
    if name == 'centre_x_1_wraps_a_row':                                 # ix == cw: the flat index is the first cell of the next row, no error
        return 3, 13, 13, [one([1, 2], [[0.75, 0.25, 1.25, 0.5], [1.0, 0.0, 1.0, 0.125]])], 0
    if name == 'centre_1_1_out_of_range':                                # the last row's ix == cw: index == cells + cw, error bit 0
        return 3, 13, 13, [one([1], [[0.75, 0.75, 1.25, 1.25]])], 1
    if name == 'three_in_one_cell':                                      # three classes accumulate, the last box's numbers stay
        return 5, 13, 13, [one([4, 0, 2], [[0.40, 0.40, 0.50, 0.50], [0.39, 0.41, 0.52, 0.49], [0.41, 0.39, 0.49, 0.53]])], 0
    if name == 'b33_ragged':                                             # empty images first and last, one image of 60 objects
        counts = [0, 3, 60] + [int(v) for v in rng.randint(0, 6, 29)] + [0]
        return 20, 13, 13, [_objects(rng, k, 20) for k in counts], 0
    if name == 'sticky_error_in_image_0':                                # image 0 holds a bad object; the others must come out right
        objs = [_objects(rng, k, 20) for k in (4, 5, 2, 7)]
        objs[0][1][2] = (0.9, 0.9, 1.3, 1.3)
        return 20, 13, 13, objs, 1
    raise KeyError(name)


LABELS = ('grid_1x1', 'grid_19x19_c80', 'grid_7x20', 'grid_20x7', 'centre_on_cell_boundary', 'zero_extent', 'centre_x_1_wraps_a_row',
          'centre_1_1_out_of_range', 'three_in_one_cell', 'b33_ragged', 'sticky_error_in_image_0')


@functools.lru_cache(maxsize=None)
def labels(name):
    classes, cw, ch, objs, err = _labels(name)
    return {'name': name, 'classes': classes, 'cw': cw, 'ch': ch, 'objs': [(_frozen(c), _frozen(b)) for c, b in objs], 'err': err}


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32)).astype(np.float32)).astype(np.float64)


def label_tolerances(box, cw, ch):
    """What the f32 chain of transform_labels may differ by from exact arithmetic on the same f32 boxes, for the box written last into
    a cell: (coords [4], offsets [2], area).

    centre = grid * (min + max) / 2 rounds twice: the sum by at most 1/2 ulp, which the product scales to less than 1 ulp of the
    product, and the product by 1/2 ulp; the halving and centre - floor(centre) are exact.  The offset therefore carries less than
    1.5 ulp of the centre = 0.75 ulp of the product grid * (min + max), the largest f32 number of the chain, and both roundings at their
    extreme do occur (grid_7x20 holds an offset 1.125 ulp of its centre away).  The bound set for these tests is 1 ulp of f32; it is
    taken at that product, where the derivation holds it.  The extent max - min rounds once and the square root
    halves a relative error: 1 ulp of the root.  Left to this file: half = extent / 2 * grid is again less than 1.5 ulp of itself, and
    offset -+ half rounds once more, so offset_xy_min / max are within 1.5 ulp(centre) + 1.5 ulp(half) + 1/2 ulp(result), bounded
    here by 4 ulp of the largest of the three; the area e_w * e_h of extents that are each the difference of two such numbers by
    |e_h| * 8 ulp_x + |e_w| * 8 ulp_y + 1 ulp of the product (the extents' own rounding is inside the 8)."""
    b = np.asarray(box, np.float32)
    grid = np.array([cw, ch], np.float32)
    centre = grid * (b[0:2] + b[2:4]) / 2
    size = b[2:4] - b[0:2]
    half = size / 2 * grid
    off = centre - np.floor(centre)
    with np.errstate(invalid='ignore'):
        coords = np.concatenate([ulp32(2 * centre), ulp32(np.sqrt(size))])
    big = 4 * ulp32(np.maximum(np.maximum(np.abs(centre), np.abs(half)), np.maximum(np.abs(off - half), np.abs(off + half))))
    extent = (off + half) - (off - half)
    area = abs(float(extent[1])) * 2 * big[0] + abs(float(extent[0])) * 2 * big[1] + float(ulp32(extent[0] * extent[1]))
    return coords, big, area


@functools.lru_cache(maxsize=None)
def labels_f64(name):
    """Per image: (the seven results of augment_ref.transform_labels, (coords [cells, 4], offsets [cells, 2], areas [cells]) tolerances,
    each cell's being those of the box written into it last)."""
    L = labels(name)
    cells = L['cw'] * L['ch']
    out = []
    for cls, box in L['objs']:
        ref = F.transform_labels(cls, box, L['classes'], L['cw'], L['ch'])
        tc, to, ta = np.zeros((cells, 4)), np.zeros((cells, 2)), np.zeros(cells)
        for c, b in zip(cls, box.astype(np.float64)):
            index = int(np.floor(L['ch'] * (b[1] + b[3]) / 2) * L['cw'] + np.floor(L['cw'] * (b[0] + b[2]) / 2))
            if 0 <= index < cells and 0 <= c < L['classes']:
                tc[index], to[index], ta[index] = label_tolerances(b, L['cw'], L['ch'])
        out.append((ref, (tc, to, ta)))
    return out


def assert_labels_match_f64(got, name, b):
    """got = (mask, prob, coords, offset_xy_min, offset_xy_max, areas) of image b in f32, any shape: mask and class bits exactly, the
    numbers within label_tolerances of the float64 reference."""
    L = labels(name)
    cells = L['cw'] * L['ch']
    (mask, prob, coords, lo, hi, areas, _), (tc, to, ta) = labels_f64(name)[b]
    g = [np.asarray(a, np.float64).reshape(r.shape) for a, r in zip(got, (mask, prob, coords, lo, hi, areas))]
    np.testing.assert_array_equal(g[0], mask, err_msg='%s[%d] mask' % (name, b))
    np.testing.assert_array_equal(g[1], prob, err_msg='%s[%d] prob' % (name, b))
    for key, a, r, t in (('coords', g[2], coords, tc), ('offset_xy_min', g[3], lo, to), ('offset_xy_max', g[4], hi, to), ('areas', g[5], areas, ta)):
        excess = np.abs(a - r) - t
        assert np.all(excess <= 0), '%s[%d] %s: %.3e beyond the tolerance at %s' % (name, b, key, excess.max(), np.unravel_index(excess.argmax(), excess.shape))
    assert cells == mask.size
