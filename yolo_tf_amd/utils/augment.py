"""On-device input pipeline: the counterpart of the reference's load_image_labels
(utils/data/__init__.py:162-175) after JPEG decode.

The reference builds this stage out of TF ops fed by an input queue; here decoded uint8 images and their raw boxes sit
in HBM and two launches produce what the training step consumes: ``yolo2_augment_images`` (crop -> bilinear resize ->
flip -> brightness / saturation / hue / contrast / noise / grayscale -> clip) and ``yolo2_transform_labels`` (boxes ->
the six label tensors, written straight into the session's label buffers).  Every random decision the reference makes
with tf.random_uniform / tf.cond is drawn here on the host, per image, from a seeded NumPy generator, in the reference's
order; the config keys are the reference's (`[data_augmentation_full]`, `[data_augmentation_resized]`, config.ini:14-28).
The box arithmetic (random_crop utils/preprocess.py:28-42, resize factor utils/data/__init__.py:63-68, flip
utils/preprocess.py:45-51, normalisation utils/data/__init__.py:171) is host NumPy in float32: a few boxes per image.

Mosaic and MixUp (new work, the reference has neither): with ``[mi355x] mosaic`` or ``mixup`` above 0 an output
image is composed of up to two layers of one or four sources each, by ONE ``yolo2_compose_images`` launch for the whole batch
(``yolo2_augment_images`` is then not launched); the layout, the box transform and filter and the order of the layers' objects are host
functions of this file, restated by tests/mosaic_ref.py.  With both keys absent or 0 nothing here is different: no draw, no buffer, the
same launch.
"""
import ctypes

import numpy as np
import torch

from .. import ops, options
from .._lib import AugmentParams, ComposeTile

FLIP, BRIGHTNESS, SATURATION, HUE, CONTRAST, NOISE, GRAY = 1, 2, 4, 8, 16, 32, 64


class AugmentConfig(object):
    """The two reference sections; missing sections / keys mean 'disabled' like `enable = 0`."""

    def __init__(self, config=None):
        def get(section, key, conv, default):
            if config is not None and config.has_section(section) and config.has_option(section, key):
                return conv(config.get(section, key))
            return default
        as_bool = lambda s: s.strip().lower() in ('1', 'true', 'yes', 'on')
        full, res = 'data_augmentation_full', 'data_augmentation_resized'
        self.full_enable = get(full, 'enable', as_bool, False)
        self.full_probability = get(full, 'enable_probability', float, 0.5)
        self.random_crop = get(full, 'random_crop', float, 0.0)
        self.resized_enable = get(res, 'enable', as_bool, False)
        self.probability = get(res, 'enable_probability', float, 0.5)
        self.flip = get(res, 'random_flip_horizontally', as_bool, False)
        self.brightness = get(res, 'random_brightness', as_bool, False)
        self.contrast = get(res, 'random_contrast', as_bool, False)
        self.saturation = get(res, 'random_saturation', as_bool, False)
        self.hue = get(res, 'random_hue', as_bool, False)
        self.noise = get(res, 'noise', as_bool, False)
        self.grayscale_probability = get(res, 'grayscale_probability', float, 0.0)
        for key, value in compose_options(config).items():
            setattr(self, key, value)

    @property
    def compose(self):
        """Whether batches go through yolo2_compose_images (mosaic or MixUp is on)."""
        return self.mosaic > 0 or self.mixup > 0


COMPOSE_RULES = (          # key, what it must satisfy, what a refusal says -- in the order the keys are checked
    ('mosaic', lambda p: 0.0 <= p <= 1.0, 'a probability per output image, in [0, 1] (0 or absent: off)'),
    ('mixup', lambda p: 0.0 <= p <= 1.0, 'a probability per output image, in [0, 1] (0 or absent: off)'),
    ('mosaic_scale', lambda lo, hi: 0.0 < lo <= hi, 'LO HI with 0 < LO <= HI, the range of a tile\'s size relative to the frame'),
    ('mosaic_center', lambda c: 0.0 <= c <= 0.5, 'the centre is drawn from [c, 1 - c] of the frame: c lies in [0, 0.5]'),
    ('mosaic_min_visible', lambda v: 0.0 <= v <= 1.0, 'the share of a box\'s area that must stay visible, in [0, 1]'),
    ('mosaic_fill', lambda g: 0.0 <= g <= 255.0, 'a grey level in [0, 255]'),
    ('mixup_alpha', lambda a: a > 0.0, 'the parameter of Beta(alpha, alpha) is positive'))
COMPOSE_DEFAULTS = {key: options.KEYS[key].default for key in ('mosaic', 'mosaic_scale', 'mosaic_center', 'mosaic_min_visible', 'mosaic_fill', 'mixup', 'mixup_alpha')}


def compose_options(config):
    """The mosaic / MixUp keys of ``[mi355x]`` as a dict of COMPOSE_DEFAULTS' keys; an absent key is its default, and ``mosaic`` / ``mixup``
    absent or 0 mean off.  An invalid value raises ValueError naming the key.  Pure host logic."""
    out = dict(COMPOSE_DEFAULTS)
    for key, ok, what in COMPOSE_RULES:
        if not options.has(config, key):
            continue
        count = np.size(COMPOSE_DEFAULTS[key])          # as many numbers as the default holds
        expected = 'expected ' + ('a number' if count == 1 else '%d numbers' % count)
        values = options.read(config, key, how='list', invalid=expected)
        if len(values) != count or not all(np.isfinite(values)):
            raise options.refusal(config, key, expected)
        if not ok(*values):
            raise options.refusal(config, key, what)
        out[key] = values[0] if count == 1 else tuple(values)
    return out


def draw_geometry(cfg, rng, src_wh, objects_coord, width, height, scale=None):
    """The geometric draws of one source, in the reference's order: the `[data_augmentation_full]` crop, the resize to the view, the
    `[data_augmentation_resized]` flip.  The view is (width, height), or with ``scale`` = (lo, hi) (a mosaic tile) that frame times
    s ~ U(lo, hi), drawn between the crop and the flip.  Returns (crop (x, y, w, h), flip, (view_w, view_h), boxes in the view's pixels)."""
    f = np.float32
    coord = np.asarray(objects_coord, f).reshape(-1, 4)
    wh = np.array(src_wh, f)
    crop = (0, 0, int(src_wh[0]), int(src_wh[1]))
    if cfg.full_enable and cfg.random_crop > 0 and len(coord) and rng.uniform() < cfg.full_probability:
        # utils/preprocess.py:28-42
        xy_min, xy_max = coord[:, :2].min(0), coord[:, 2:].max(0)
        shrink = rng.uniform(0, cfg.random_crop, 4).astype(f) * np.concatenate([xy_min, wh - xy_max]).astype(f)
        _xy_min = shrink[:2]
        _wh = wh - shrink[2:] - _xy_min
        coord = coord - np.tile(_xy_min, 2)
        crop = (int(_xy_min[0]), int(_xy_min[1]), max(int(_wh[0]), 1), max(int(_wh[1]), 1))
        wh = _wh
    if scale is not None:
        s = rng.uniform(scale[0], scale[1])
        width, height = max(1, int(round(s * width))), max(1, int(round(s * height)))
    coord = coord * np.tile(np.array([width, height], f) / wh, 2)            # resize_image_objects
    flip = False
    if cfg.resized_enable and cfg.flip and rng.uniform() < 0.5:              # random_flip_horizontally, probability 0.5
        flip = True
        w = f(width)
        coord = np.stack([w - coord[:, 2], coord[:, 1], w - coord[:, 0], coord[:, 3]], 1)
    return crop, flip, (width, height), coord


def draw_photo(cfg, rng, p):
    """The photometric draws of one output image into p (flags and scalars), in the reference's order."""
    if cfg.resized_enable:
        if cfg.brightness and rng.uniform() < cfg.probability:
            p['flags'] |= BRIGHTNESS
            p['brightness'] = float(rng.uniform(-63, 63))
        if cfg.saturation and rng.uniform() < cfg.probability:
            p['flags'] |= SATURATION
            p['saturation'] = float(rng.uniform(0.5, 1.5))
        if cfg.hue and rng.uniform() < cfg.probability:
            p['flags'] |= HUE
            p['hue'] = float(rng.uniform(-0.032, 0.032))
        if cfg.contrast and rng.uniform() < cfg.probability:
            p['flags'] |= CONTRAST
            p['contrast'] = float(rng.uniform(0.5, 1.5))
        if cfg.noise and rng.uniform() < cfg.probability:
            p['flags'] |= NOISE
            p['noise_scale'] = float(rng.uniform(5, 15))
            p['noise_seed'] = int(rng.randint(0, 2 ** 31 - 1)) * 4294967291 + int(rng.randint(0, 2 ** 31 - 1))
        if cfg.grayscale_probability > 0 and rng.uniform() < cfg.grayscale_probability:
            p['flags'] |= GRAY
    return p


def _photo_defaults():
    return dict(flags=0, brightness=0.0, saturation=1.0, hue=0.0, contrast=1.0, noise_scale=0.0, noise_seed=0)


def draw(cfg, rng, src_wh, objects_coord, width, height):
    """One image's random decisions + the transformed boxes.

    src_wh = (w, h) of the decoded image, objects_coord [K,4] float pixels (xmin, ymin, xmax, ymax).
    Returns (dict for AugmentParams: crop, flags, scalars, seed; boxes normalised to [0,1] as float32 [K,4])."""
    f = np.float32
    crop, flip, _, coord = draw_geometry(cfg, rng, src_wh, objects_coord, width, height)
    p = dict(_photo_defaults(), crop=crop, flags=FLIP if flip else 0)
    draw_photo(cfg, rng, p)
    coord = (coord / np.array([width, height, width, height], f)).astype(f)  # utils/data/__init__.py:171
    return p, coord


# ---- mosaic and MixUp: the host part ------------------------------------------------------------------------
def mosaic_layout(fx, fy, width, height):
    """The centre (cx, cy) = (int(fx * width), int(fy * height)) and the four half-open rectangles (x0, y0, x1, y1) of the quadrants
    top-left, top-right, bottom-left, bottom-right: a partition of the frame for every centre in it (a quadrant may be empty)."""
    cx, cy = int(fx * width), int(fy * height)
    return cx, cy, [(0, 0, cx, cy), (cx, 0, width, cy), (0, cy, cx, height), (cx, cy, width, height)]


def mosaic_origin(q, cx, cy, view_w, view_h):
    """Where view pixel (0, 0) of quadrant q lands: the view's corner nearest the centre touches the centre."""
    return (cx - view_w if q in (0, 2) else cx, cy - view_h if q in (0, 1) else cy)


def tile_boxes(coord, origin, rect, view_wh, min_visible, width, height):
    """Boxes in a view's pixels -> (indices kept, their boxes normalised by the frame): move by the origin, clip to the tile's rectangle
    intersected with the view's extent, drop what is left narrower or lower than 2 px or with less than ``min_visible`` of its area."""
    f = np.float32
    coord = np.asarray(coord, f).reshape(-1, 4) + np.array([origin[0], origin[1], origin[0], origin[1]], f)
    lo = np.array([max(rect[0], origin[0]), max(rect[1], origin[1])], f)
    hi = np.array([min(rect[2], origin[0] + view_wh[0]), min(rect[3], origin[1] + view_wh[1])], f)
    clipped = np.concatenate([np.minimum(np.maximum(coord[:, :2], lo), hi), np.minimum(np.maximum(coord[:, 2:], lo), hi)], 1)
    full_wh = coord[:, 2:] - coord[:, :2]
    wh = clipped[:, 2:] - clipped[:, :2]
    if hi[0] <= lo[0] or hi[1] <= lo[1]:
        wh = np.zeros_like(wh)                       # nothing of the view shows in the rectangle
    keep = (wh[:, 0] >= f(2)) & (wh[:, 1] >= f(2)) & (wh[:, 0] * wh[:, 1] >= f(min_visible) * (full_wh[:, 0] * full_wh[:, 1]))
    kept = np.nonzero(keep)[0]
    return kept, (clipped[kept] / np.array([width, height, width, height], f)).astype(f)


def draw_layer(cfg, rng, index, sizes, objects, width, height):
    """One layer of an output image whose first source is dataset image ``index``: a mosaic with probability cfg.mosaic, otherwise the
    ordinary image as one full-frame tile.  Returns dict(tiles: dicts of index, crop, view, origin, rect, flip; classes; boxes)."""
    if cfg.mosaic > 0 and rng.uniform() < cfg.mosaic:
        c = cfg.mosaic_center
        fx, fy = rng.uniform(c, 1 - c), rng.uniform(c, 1 - c)                # fractions: no draw depends on the output size
        cx, cy, rects = mosaic_layout(fx, fy, width, height)
        indices = [int(index)] + [int(i) for i in rng.randint(0, len(sizes), 3)]
        tiles, cls, box = [], [], []
        for q, i in enumerate(indices):
            crop, flip, view, coord = draw_geometry(cfg, rng, sizes[i], objects[i][1], width, height, scale=cfg.mosaic_scale)
            origin = mosaic_origin(q, cx, cy, *view)
            kept, boxes = tile_boxes(coord, origin, rects[q], view, cfg.mosaic_min_visible, width, height)
            tiles.append(dict(index=i, crop=crop, view=view, origin=origin, rect=rects[q], flip=flip))
            cls.append(objects[i][0][kept])
            box.append(boxes)
        return dict(tiles=tiles, classes=np.concatenate(cls).astype(np.int32), boxes=np.concatenate(box).astype(np.float32).reshape(-1, 4),
                    mosaic=True, center=(fx, fy))
    f = np.float32
    crop, flip, view, coord = draw_geometry(cfg, rng, sizes[index], objects[index][1], width, height)
    boxes = (coord / np.array([width, height, width, height], f)).astype(f)
    tile = dict(index=int(index), crop=crop, view=view, origin=(0, 0), rect=(0, 0, width, height), flip=flip)
    return dict(tiles=[tile], classes=np.asarray(objects[index][0], np.int32), boxes=boxes.reshape(-1, 4), mosaic=False, center=None)


def merge_layers(layers, lam):
    """The objects of an output image: the lighter layer's first, so that in a contested cell the heavier image's object is written
    last and wins (``lam`` = the weight of layer 0; equal weights count layer 0 as the heavier)."""
    order = layers if len(layers) == 1 else ([layers[1], layers[0]] if lam >= 0.5 else [layers[0], layers[1]])
    return (np.concatenate([l['classes'] for l in order]).astype(np.int32),
            np.concatenate([l['boxes'] for l in order]).astype(np.float32).reshape(-1, 4))


def draw_composite(cfg, rng, index, sizes, objects, width, height):
    """One output image of the compose path: layer 0 from dataset image ``index``; with probability cfg.mixup a second layer from a
    further index and lam ~ Beta(alpha, alpha), the weight of layer 0 (rounded to f32, as the device receives it); then the photometric
    draws, once.  Returns dict(layers, lam, photo, classes, boxes)."""
    layers, lam = [draw_layer(cfg, rng, index, sizes, objects, width, height)], 1.0
    if cfg.mixup > 0 and rng.uniform() < cfg.mixup:
        second = int(rng.randint(0, len(sizes)))
        layers.append(draw_layer(cfg, rng, second, sizes, objects, width, height))
        lam = float(np.float32(rng.beta(cfg.mixup_alpha, cfg.mixup_alpha)))
    photo = draw_photo(cfg, rng, _photo_defaults())
    cls, box = merge_layers(layers, lam)
    return dict(layers=layers, lam=lam, photo=photo, classes=cls, boxes=box)


class ComposeBatch(object):
    """What ``assemble`` hands to ``launch`` when mosaic or MixUp is on: the ctypes arrays of one yolo2_compose_images call."""

    def __init__(self, tiles, photo, mix, L, T, images):
        self.tiles, self.photo, self.mix, self.L, self.T, self.images = tiles, photo, mix, L, T, images


class DeviceInputPipeline(object):
    """Keeps a dataset of decoded images in HBM and assembles training batches there.

    images: list of uint8 [h, w, 3] arrays (any sizes); objects: list of (classes int [K], coords float [K,4] pixels).
    ``next(session)`` fills the session's label buffers in place and returns the f32 [B,H,W,3] image batch (0..255) that
    ``TrainSession.step`` standardises.

    ``sizes``: optional list of (width, height) for multi-scale training; ``downsampling`` = (dw, dh) of the network (default: what width /
    cell_width and height / cell_height say).  The output is then allocated once, for the largest size, and ``next(session)`` produces the
    batch and the labels for ``session.size``: a contiguous [B,h,w,3] view at the start of that buffer, on a grid of w // dw x h // dh.  The
    host draws do not depend on the output size, so a size change never shifts the random stream.  Without ``sizes`` there is one size and
    one buffer of exactly its shape.

    With ``[mi355x] mosaic`` or ``mixup`` on (cfg.compose) the batch is composed by ``yolo2_compose_images`` instead; the further dataset
    indices and every other extra decision come from the same generator, as fractions of the frame."""

    def __init__(self, images, objects, batch, width, height, classes, cell_width, cell_height, config=None, seed=0, rank=0, world=1,
                 sizes=None, downsampling=None):
        assert len(images) == len(objects) and len(images) > 0
        self.cfg = config if isinstance(config, AugmentConfig) else AugmentConfig(config)
        self.B, self.W, self.H, self.classes = batch, width, height, classes
        self.cell_width, self.cell_height = cell_width, cell_height
        self.rng = np.random.RandomState(seed)
        self.rank, self.world = rank, world
        self.sizes = [(im.shape[1], im.shape[0]) for im in images]
        offsets = np.cumsum([0] + [im.shape[0] * im.shape[1] * 3 for im in images])
        self.offsets = offsets[:-1]
        packed = np.concatenate([np.ascontiguousarray(im, np.uint8).reshape(-1) for im in images])
        self.src = torch.from_numpy(packed).cuda()
        self.objects = [(np.asarray(c, np.int32).reshape(-1), np.asarray(b, np.float32).reshape(-1, 4)) for c, b in objects]
        dev = self.src.device
        self._views = None
        if sizes:
            self.downsampling = tuple(int(d) for d in downsampling) if downsampling is not None else (width // cell_width, height // cell_height)
            assert (cell_width * self.downsampling[0], cell_height * self.downsampling[1]) == (width, height)
            every = sorted(set((int(w), int(h)) for w, h in sizes) | {(width, height)})
            assert all(w % self.downsampling[0] == 0 and h % self.downsampling[1] == 0 for w, h in every), 'sizes must be multiples of the downsampling'
            self.buffer = torch.zeros(batch * max(w * h for w, h in every) * 3, dtype=torch.float32, device=dev)
            self._views = {(w, h): self.buffer[:batch * h * w * 3].view(batch, h, w, 3) for w, h in every}
            self.out = self._views[(width, height)]
        else:
            self.out = self.buffer = torch.zeros(batch, height, width, 3, dtype=torch.float32, device=dev)
        self.ws = torch.zeros(3 * batch, dtype=torch.float64, device=dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)

    def sample(self):
        idx = self.rng.randint(0, len(self.sizes), self.B * self.world)
        return idx[self.rank::self.world]

    def assemble(self, indices):
        """Host part: random draws + box transforms.  Returns (AugmentParams array, classes, coords, first_object); with mosaic or MixUp
        on, a ComposeBatch in the array's place."""
        if self.cfg.compose:
            return self.assemble_composites(indices)
        arr = (AugmentParams * self.B)()
        cls, box, first = [], [], [0]
        for d, i in zip(arr, indices):
            c, b = self.objects[i]
            p, nb = draw(self.cfg, self.rng, self.sizes[i], b, self.W, self.H)
            d.src_offset = int(self.offsets[i])
            d.src_w, d.src_h = self.sizes[i]
            d.crop_x, d.crop_y, d.crop_w, d.crop_h = p['crop']
            d.flags = p['flags']
            d.brightness, d.saturation, d.hue, d.contrast = p['brightness'], p['saturation'], p['hue'], p['contrast']
            d.noise_scale, d.noise_seed = p['noise_scale'], p['noise_seed'] & (2 ** 64 - 1)
            cls.append(c)
            box.append(nb)
            first.append(first[-1] + len(c))
        return arr, np.concatenate(cls).astype(np.int32), np.concatenate(box).astype(np.float32).reshape(-1, 4), np.asarray(first, np.int32)

    def assemble_composites(self, indices):
        """``assemble`` of the compose path: L = 2 layers when MixUp is on, T = 4 tiles when mosaic is on, unused slots empty."""
        L, T = 2 if self.cfg.mixup > 0 else 1, 4 if self.cfg.mosaic > 0 else 1
        tiles, photo, mix = (ComposeTile * (self.B * L * T))(), (AugmentParams * self.B)(), (ctypes.c_float * self.B)()
        images, cls, box, first = [], [], [], [0]
        for b, i in enumerate(indices):
            im = draw_composite(self.cfg, self.rng, int(i), self.sizes, self.objects, self.W, self.H)
            for l, layer in enumerate(im['layers']):
                for k, t in enumerate(layer['tiles']):
                    d = tiles[(b * L + l) * T + k]
                    d.src_offset = int(self.offsets[t['index']])
                    d.src_w, d.src_h = self.sizes[t['index']]
                    d.crop_x, d.crop_y, d.crop_w, d.crop_h = t['crop']
                    d.view_w, d.view_h = t['view']
                    d.origin_x, d.origin_y = t['origin']
                    d.x0, d.y0, d.x1, d.y1 = t['rect']
                    d.flip = int(t['flip'])
            p, d = im['photo'], photo[b]
            d.flags = p['flags']
            d.brightness, d.saturation, d.hue, d.contrast = p['brightness'], p['saturation'], p['hue'], p['contrast']
            d.noise_scale, d.noise_seed = p['noise_scale'], p['noise_seed'] & (2 ** 64 - 1)
            mix[b] = im['lam']
            images.append(im)
            cls.append(im['classes'])
            box.append(im['boxes'])
            first.append(first[-1] + len(im['classes']))
        return (ComposeBatch(tiles, photo, mix, L, T, images), np.concatenate(cls).astype(np.int32),
                np.concatenate(box).astype(np.float32).reshape(-1, 4), np.asarray(first, np.int32))

    def launch(self, arr, cls, box, first, labels):
        """Device part: both kernels; ``labels`` = the six device tensors of the loss (TrainSession.labels)."""
        if isinstance(arr, ComposeBatch):
            upload = lambda a: torch.frombuffer(bytearray(bytes(a)), dtype=torch.uint8).cuda()
            params = (upload(arr.tiles), upload(arr.photo), upload(arr.mix))
            any_contrast = any(a.flags & CONTRAST for a in arr.photo)
            ops.compose_images(self.src, params[0], params[1], params[2], self.ws, self.out, self.B, arr.L, arr.T, self.H, self.W,
                               self.cfg.mosaic_fill, any_contrast)
        else:
            params = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
            any_contrast = any(a.flags & CONTRAST for a in arr)
            ops.augment_images(self.src, params, self.ws, self.out, self.B, self.H, self.W, any_contrast)
        n = max(len(cls), 1)
        cls_d = torch.from_numpy(np.resize(cls, n) if len(cls) else np.zeros(1, np.int32)).cuda()
        box_d = torch.from_numpy(box if len(box) else np.zeros((1, 4), np.float32)).cuda()
        first_d = torch.from_numpy(first).cuda()
        # the flag is sticky (the kernel ORs into it): check() reports a bad object of ANY batch since the last check
        ops.transform_labels(cls_d, box_d, first_d, *labels, self.B, self.classes, self.cell_width, self.cell_height, self.err)
        self._keep = (params, cls_d, box_d, first_d)      # alive until the next launch (asynchronous kernels)
        return self.out

    def set_size(self, width, height):
        """Multi-scale: the size (one of ``sizes``) of the batches and label grids that follow."""
        if (width, height) == (self.W, self.H):
            return
        if self._views is None or (width, height) not in self._views:
            raise KeyError('input size %dx%d is not one of the sizes the pipeline was built with' % (width, height))
        self.W, self.H = width, height
        self.cell_width, self.cell_height = width // self.downsampling[0], height // self.downsampling[1]
        self.out = self._views[(width, height)]

    def next(self, session):
        if self._views is not None:
            self.set_size(*session.size)
        arr, cls, box, first = self.assemble(self.sample())
        return self.launch(arr, cls, box, first, session.labels)

    def check(self):
        """Raises like the reference would (IndexError / AssertionError in transform_labels); synchronises."""
        e = int(self.err.item())
        self.err.zero_()
        if e & 1:
            raise IndexError('transform_labels: object outside the grid or class id out of range')
        if e & 2:
            raise AssertionError('transform_labels: negative box extent')

