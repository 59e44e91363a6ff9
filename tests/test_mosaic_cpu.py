"""Mosaic and MixUp, the host part (yolo_tf_amd/utils/augment.py), without a GPU: the layout, the box rule on cases
worked out by hand, the order of the layers' objects, the random stream (untouched when the keys are off, independent of the frame size)
and the validation of the `[mi355x]` keys.  Every function is also held to its restatement in tests/mosaic_ref.py."""
import configparser
import os

import numpy as np
import pytest

import augment_ref as F
import mosaic_ref as M
from oracle import yolo2_ref as R
from yolo_tf_amd.utils import augment as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def config(**keys):
    """The repository's config.ini (both augmentation sections enabled) with `[mi355x]` keys set."""
    ini = configparser.ConfigParser()
    ini.read(os.path.join(ROOT, 'config.ini'))
    for k, v in keys.items():
        ini.set('mi355x', k, str(v))
    return ini


def dataset(seed, n=12):
    """Seeded sources of 50 .. 150 px with 1 .. 4 boxes each: centres over the middle 70 % of the image, 8 .. 30 % of it wide and high."""
    r = np.random.RandomState(seed)
    sizes = [(int(r.randint(50, 150)), int(r.randint(50, 150))) for _ in range(n)]
    objects = []
    for w, h in sizes:
        k = r.randint(1, 5)
        cx, cy = r.uniform(.15 * w, .85 * w, k), r.uniform(.15 * h, .85 * h, k)
        bw, bh = r.uniform(.08 * w, .3 * w, k), r.uniform(.08 * h, .3 * h, k)
        objects.append((r.randint(0, 20, k).astype(np.int32), np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1).astype(f32)))
    return sizes, objects


# ---- layout ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [(45, 31), (1, 17), (128, 96)])
def test_partition(size):
    """The four rectangles cover every pixel exactly once, for every centre the draw can give.  cx = int(fx * W) with fx in [c, 1 - c]: the
    product lies in [c * W, (1 - c) * W] and the truncation can only take cx down to floor(c * W) (W = 1 gives cx = 0)."""
    W, H = size
    rng = np.random.RandomState(W * 1000 + H)
    c = A.COMPOSE_DEFAULTS['mosaic_center']
    for _ in range(200):
        fx, fy = rng.uniform(c, 1 - c), rng.uniform(c, 1 - c)
        cx, cy, rects = A.mosaic_layout(fx, fy, W, H)
        assert (cx, cy, rects) == M.layout(fx, fy, W, H)
        assert c * W <= fx * W <= (1 - c) * W and c * H <= fy * H <= (1 - c) * H
        assert np.floor(c * W) <= cx <= (1 - c) * W and np.floor(c * H) <= cy <= (1 - c) * H
        count = np.zeros((H, W), np.int32)
        for x0, y0, x1, y1 in rects:
            assert 0 <= x0 <= x1 <= W and 0 <= y0 <= y1 <= H
            count[y0:y1, x0:x1] += 1
        assert (count == 1).all()
        for q in range(4):
            assert A.mosaic_origin(q, cx, cy, 13, 7) == M.origin(q, cx, cy, 13, 7)
    assert A.mosaic_origin(0, 40, 30, 60, 50) == (-20, -20) and A.mosaic_origin(1, 40, 30, 60, 50) == (40, -20)
    assert A.mosaic_origin(2, 40, 30, 60, 50) == (-20, 30) and A.mosaic_origin(3, 40, 30, 60, 50) == (40, 30)


# ---- the box rule, by hand: a 100 x 80 frame with the centre at (40, 30) ------------------------------------------------------------------
W, H, CX, CY = 100, 80, 40, 30
Q0, Q3 = (0, 0, CX, CY), (CX, CY, W, H)
BOX_CASES = {
    # name: (box in the view's pixels, flip, view, origin, rectangle, min_visible, expected box in the frame's pixels or None = dropped)
    'inside_q3_translated_only': ((5, 6, 25, 26), False, (50, 40), (40, 30), Q3, 0.25, (45, 36, 65, 56)),
    # q0's view ends at the centre; a box that reaches 10 px beyond its image straddles the centre line and is cut there
    'straddles_cx_in_q0': ((30, 25, 70, 45), False, (60, 50), (-20, -20), Q0, 0.25, (10, 5, 40, 25)),
    # mirrored in the 60 px view it is (-10, 25, 30, 45) -> (-30, 5, 10, 25) in the frame -> cut at the frame's edge: 10 of 40 px
    'the_same_flipped': ((30, 25, 70, 45), True, (60, 50), (-20, -20), Q0, 0.25, (0, 5, 10, 25)),
    # (24, 25, 64, 45) - (60, 20) = (-36, 5, 4, 25): 4 x 20 = 80 px^2 of 800
    'ten_percent_visible': ((24, 25, 64, 45), False, (100, 50), (-60, -20), Q0, 0.25, None),
    # (-30, 5, 10, 25): 10 x 20 = 200 px^2 = 0.25 * 800 exactly: the rule is >=
    'exactly_min_visible': ((30, 25, 70, 45), False, (100, 50), (-60, -20), Q0, 0.25, (0, 5, 10, 25)),
    'just_below_min_visible': ((29.5, 25, 69.5, 45), False, (100, 50), (-60, -20), Q0, 0.25, None),
    # min_visible 0 leaves the 2 px rule alone: (58, 25, 61.9, 45) -> (-2, 5, 1.9, 25) -> 1.9 px wide
    'sliver_1p9_px': ((58, 25, 61.9, 45), False, (100, 50), (-60, -20), Q0, 0.0, None),
    'sliver_2_px': ((58, 25, 62, 45), False, (100, 50), (-60, -20), Q0, 0.0, (0, 5, 2, 25)),
    'sliver_1p9_px_high': ((70, 16, 90, 21.9), False, (100, 50), (-60, -20), Q0, 0.0, None),
    # a 30 x 20 view in the 60 x 50 quadrant: the box is cut at the view's edge (70), not at the rectangle's (100)
    'view_smaller_than_quadrant': ((10, 5, 40, 18), False, (30, 20), (40, 30), Q3, 0.25, (50, 35, 70, 48)),
    'quadrant_empty': ((5, 6, 25, 26), False, (50, 40), (0, 30), (0, 30, 0, 80), 0.0, None),
}


@pytest.mark.parametrize('name', sorted(BOX_CASES))
def test_box_case(name):
    box, flip, view, origin, rect, min_visible, expected = BOX_CASES[name]
    coord = np.array([box], f32)
    if flip:
        coord = R.flip_coords(coord, view[0])
    for fn in (A.tile_boxes, M.tile_boxes):
        kept, got = fn(coord, origin, rect, view, min_visible, W, H)
        if expected is None:
            assert len(kept) == 0 and got.shape == (0, 4)
        else:
            assert list(kept) == [0]
            assert got.dtype == np.float32
            np.testing.assert_array_equal(got[0], np.array(expected, f32) / np.array([W, H, W, H], f32))


def test_box_rule_keeps_the_order_of_the_survivors():
    boxes = np.array([BOX_CASES[k][0] for k in ('exactly_min_visible', 'ten_percent_visible', 'sliver_2_px', 'just_below_min_visible')], f32)
    for fn in (A.tile_boxes, M.tile_boxes):
        kept, got = fn(boxes, (-60, -20), Q0, (100, 50), 0.25, W, H)
        assert list(kept) == [0, 2] and len(got) == 2           # (the 2 px sliver shows 2 of its 4 px: half of its area)
        kept, _ = fn(boxes, (-60, -20), Q0, (100, 50), 0.0, W, H)
        assert list(kept) == [0, 1, 2, 3]


# ---- labels ---------------------------------------------------------------------------------------------------------------------------
def test_no_label_errors_over_500_mosaics():
    """No mosaic raises transform_labels' error flag, and the test is not passing on empty label sets: at least half of all source boxes
    survive.  With the default `mosaic_scale = 0.5 1.5` that share cannot be had from any choice of boxes: a quadrant shows the part of its view
    next to the centre, min(1, fx / s) of it per axis on average 0.6, so about 0.39 of the boxes of ANY placement survive (measured:
    0.386 with centred boxes, 0.391 with these).  The test therefore narrows the range to 0.5 .. 0.75, where a tile mostly fits its
    quadrant; the boxes are dataset()'s.  Measured surviving share: 0.703 of 5290 boxes."""
    cfg = A.AugmentConfig(config(mosaic=1, mosaic_scale='0.5 0.75'))
    sizes, objects = dataset(5)
    rng, ref_rng = np.random.RandomState(1), np.random.RandomState(1)
    total = kept = 0
    for _ in range(500):
        i = int(rng.randint(0, len(sizes)))
        assert i == int(ref_rng.randint(0, len(sizes)))
        im = A.draw_composite(cfg, rng, i, sizes, objects, 96, 64)
        ref = M.draw_image(cfg, ref_rng, i, sizes, objects, 96, 64)
        np.testing.assert_array_equal(im['boxes'], ref['boxes'])
        np.testing.assert_array_equal(im['classes'], ref['classes'])
        assert len(im['layers']) == 1 and len(im['layers'][0]['tiles']) == 4
        total += sum(len(objects[t['index']][0]) for t in im['layers'][0]['tiles'])
        kept += len(im['classes'])
        assert F.transform_labels(im['classes'], im['boxes'], 20, 3, 2)[6] == 0
        if len(im['boxes']):
            centre = (im['boxes'][:, :2] + im['boxes'][:, 2:]) / 2
            assert (centre > 0).all() and (centre < 1).all()
    print('surviving share: %.3f of %d boxes' % (kept / total, total))
    assert kept >= 0.5 * total


# ---- the random stream ----------------------------------------------------------------------------------------------------------------
def _parent_draw(cfg, rng, src_wh, objects_coord, width, height):
    """`draw` as it stood before mosaic and MixUp, word for word: what the stream and the results are compared against."""
    f = np.float32
    coord = np.asarray(objects_coord, f).reshape(-1, 4)
    wh = np.array(src_wh, f)
    crop = (0, 0, int(src_wh[0]), int(src_wh[1]))
    if cfg.full_enable and cfg.random_crop > 0 and len(coord) and rng.uniform() < cfg.full_probability:
        xy_min, xy_max = coord[:, :2].min(0), coord[:, 2:].max(0)
        shrink = rng.uniform(0, cfg.random_crop, 4).astype(f) * np.concatenate([xy_min, wh - xy_max]).astype(f)
        _xy_min = shrink[:2]
        _wh = wh - shrink[2:] - _xy_min
        coord = coord - np.tile(_xy_min, 2)
        crop = (int(_xy_min[0]), int(_xy_min[1]), max(int(_wh[0]), 1), max(int(_wh[1]), 1))
        wh = _wh
    coord = coord * np.tile(np.array([width, height], f) / wh, 2)
    p = dict(crop=crop, flags=0, brightness=0.0, saturation=1.0, hue=0.0, contrast=1.0, noise_scale=0.0, noise_seed=0)
    if cfg.resized_enable:
        if cfg.flip and rng.uniform() < 0.5:
            p['flags'] |= A.FLIP
            w = f(width)
            coord = np.stack([w - coord[:, 2], coord[:, 1], w - coord[:, 0], coord[:, 3]], 1)
        if cfg.brightness and rng.uniform() < cfg.probability:
            p['flags'] |= A.BRIGHTNESS
            p['brightness'] = float(rng.uniform(-63, 63))
        if cfg.saturation and rng.uniform() < cfg.probability:
            p['flags'] |= A.SATURATION
            p['saturation'] = float(rng.uniform(0.5, 1.5))
        if cfg.hue and rng.uniform() < cfg.probability:
            p['flags'] |= A.HUE
            p['hue'] = float(rng.uniform(-0.032, 0.032))
        if cfg.contrast and rng.uniform() < cfg.probability:
            p['flags'] |= A.CONTRAST
            p['contrast'] = float(rng.uniform(0.5, 1.5))
        if cfg.noise and rng.uniform() < cfg.probability:
            p['flags'] |= A.NOISE
            p['noise_scale'] = float(rng.uniform(5, 15))
            p['noise_seed'] = int(rng.randint(0, 2 ** 31 - 1)) * 4294967291 + int(rng.randint(0, 2 ** 31 - 1))
        if cfg.grayscale_probability > 0 and rng.uniform() < cfg.grayscale_probability:
            p['flags'] |= A.GRAY
    coord = (coord / np.array([width, height, width, height], f)).astype(f)
    return p, coord


def _host_pipeline(cfg, sizes, objects, batch, width, height, seed):
    """A DeviceInputPipeline with its host state only: `sample` and `assemble` touch nothing else."""
    pipe = A.DeviceInputPipeline.__new__(A.DeviceInputPipeline)
    pipe.cfg, pipe.B, pipe.W, pipe.H = cfg, batch, width, height
    pipe.rng, pipe.rank, pipe.world = np.random.RandomState(seed), 0, 1
    pipe.sizes, pipe.objects = sizes, objects
    pipe.offsets = np.cumsum([0] + [w * h * 3 for w, h in sizes])[:-1]
    return pipe


@pytest.mark.parametrize('keys', [dict(), dict(mosaic=0, mixup=0), dict(mosaic='0.0', mosaic_scale='0.7 0.9', mixup_alpha=3)])
def test_unchanged_when_off(keys, monkeypatch):
    """Both keys absent or 0: `assemble` takes the draws of the parent's `draw`, image for image, returns its parameters and boxes and
    leaves the generator in the state `draw` alone leaves it in; nothing of the compose path is reached."""
    cfg = A.AugmentConfig(config(**keys))
    assert not cfg.compose and cfg.full_enable and cfg.resized_enable
    monkeypatch.setattr(A, 'draw_composite', lambda *a, **k: pytest.fail('the compose path was taken'))
    sizes, objects = dataset(7)
    pipe = _host_pipeline(cfg, sizes, objects, 8, 96, 64, seed=11)
    ref = np.random.RandomState(11)
    for _ in range(5):                                                # N = 40 images
        idx = pipe.sample()
        ref_idx = ref.randint(0, len(sizes), 8)
        np.testing.assert_array_equal(idx, ref_idx)
        arr, cls, box, first = pipe.assemble(idx)
        assert not isinstance(arr, A.ComposeBatch)
        for b, i in enumerate(ref_idx):
            p, nb = _parent_draw(cfg, ref, sizes[i], objects[i][1], 96, 64)
            np.testing.assert_array_equal(box[first[b]:first[b + 1]], nb)
            a = arr[b]
            assert (a.crop_x, a.crop_y, a.crop_w, a.crop_h) == p['crop'] and a.flags == p['flags']
            assert (a.brightness, a.saturation, a.hue, a.contrast, a.noise_scale) == tuple(f32(p[k]) for k in ('brightness', 'saturation', 'hue', 'contrast', 'noise_scale'))
            assert a.noise_seed == p['noise_seed'] & (2 ** 64 - 1)
        assert all(np.array_equal(x, y) for x, y in zip(pipe.rng.get_state()[1:], ref.get_state()[1:]))


def _decisions(im):
    layers = [[(t['index'], t['crop'], t['flip']) for t in l['tiles']] for l in im['layers']]
    return layers, [l['center'] for l in im['layers']], im['lam'], im['photo']


def test_size_independence():
    """The same seed at 64 x 48 and at 128 x 96: the same fractions, dataset indices, crops, flips, lam and photometric draws, and the
    same generator state afterwards; only what is measured in the frame's pixels follows the size."""
    cfg = A.AugmentConfig(config(mosaic=0.7, mixup=0.5))
    sizes, objects = dataset(9)
    small, large = np.random.RandomState(4), np.random.RandomState(4)
    mosaics = mixed = 0
    for k in range(60):
        a = A.draw_composite(cfg, small, k % len(sizes), sizes, objects, 64, 48)
        b = A.draw_composite(cfg, large, k % len(sizes), sizes, objects, 128, 96)
        assert _decisions(a) == _decisions(b)
        mosaics += a['layers'][0]['mosaic']
        mixed += len(a['layers']) == 2
        for la, lb in zip(a['layers'], b['layers']):                         # what is in pixels follows from the fractions and the size alone
            if la['mosaic']:
                assert [t['rect'] for t in la['tiles']] == M.layout(*la['center'], 64, 48)[2]
                assert [t['rect'] for t in lb['tiles']] == M.layout(*lb['center'], 128, 96)[2]
            else:
                assert la['tiles'][0]['rect'] == (0, 0, 64, 48) and lb['tiles'][0]['rect'] == (0, 0, 128, 96)
    assert 0 < mosaics < 60 and 0 < mixed < 60
    assert all(np.array_equal(x, y) for x, y in zip(small.get_state()[1:], large.get_state()[1:]))


def test_stream_matches_the_specification():
    cfg = A.AugmentConfig(config(mosaic=0.6, mixup=0.5, mixup_alpha=0.8))
    sizes, objects = dataset(3)
    ours, spec = np.random.RandomState(2), np.random.RandomState(2)
    for k in range(200):
        a = A.draw_composite(cfg, ours, k % len(sizes), sizes, objects, 96, 64)
        b = M.draw_image(cfg, spec, k % len(sizes), sizes, objects, 96, 64)
        assert a['lam'] == b['lam'] and len(a['layers']) == len(b['layers'])
        np.testing.assert_array_equal(a['boxes'], b['boxes'])
        np.testing.assert_array_equal(a['classes'], b['classes'])
        for la, lb in zip(a['layers'], b['layers']):
            assert [{k: t[k] for k in s} for t, s in zip(la['tiles'], lb)] == lb
        for key in ('brightness', 'saturation', 'hue', 'contrast'):
            assert (b['photo'][key] is None) == (not a['photo']['flags'] & getattr(A, key.upper()))
            assert b['photo'][key] is None or b['photo'][key] == a['photo'][key]
    assert all(np.array_equal(x, y) for x, y in zip(ours.get_state()[1:], spec.get_state()[1:]))


# ---- MixUp ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lam, first', [(0.3, 0), (0.49999, 0), (0.5, 1), (0.7, 1), (1.0, 1)])
def test_mixup_order(lam, first):
    """The heavier layer's objects come last (transform_labels: the last object of a cell wins); lam is the weight of layer 0."""
    layers = [dict(classes=np.array([1, 2], np.int32), boxes=np.array([[.1, .1, .3, .3], [.2, .2, .6, .6]], f32)),
              dict(classes=np.array([7], np.int32), boxes=np.array([[.1, .1, .3, .3]], f32))]
    cls, box = A.merge_layers(layers, lam)
    order = (0, 1) if first == 0 else (1, 0)
    assert order == M.layer_order(lam)
    np.testing.assert_array_equal(cls, np.concatenate([layers[i]['classes'] for i in order]))
    np.testing.assert_array_equal(box, np.concatenate([layers[i]['boxes'] for i in order]))
    # the contested cell (both layers hold the box (.1, .1, .3, .3)): the heavier layer's class is the one written last
    assert cls[np.nonzero((box == box[0]).all(1))[0][-1]] == (7 if lam < 0.5 else 1)
    one = A.merge_layers(layers[:1], 1.0)
    np.testing.assert_array_equal(one[0], layers[0]['classes'])


def test_mixup_draws_both_sides_of_one_half():
    cfg = A.AugmentConfig(config(mixup=1))
    sizes, objects = dataset(3)
    rng = np.random.RandomState(0)
    seen = set()
    for k in range(40):
        im = A.draw_composite(cfg, rng, k % len(sizes), sizes, objects, 96, 64)
        assert len(im['layers']) == 2 and 0 < im['lam'] < 1 and not im['layers'][0]['mosaic']
        heavy = im['layers'][0 if im['lam'] >= 0.5 else 1]
        n = len(heavy['classes'])
        np.testing.assert_array_equal(im['classes'][len(im['classes']) - n:], heavy['classes'])
        np.testing.assert_array_equal(im['boxes'][len(im['boxes']) - n:], heavy['boxes'])
        seen.add(im['lam'] >= 0.5)
    assert seen == {True, False}


# ---- configuration --------------------------------------------------------------------------------------------------------------------
def test_config_defaults_and_values():
    cfg = A.AugmentConfig(config())
    assert (cfg.mosaic, cfg.mixup, cfg.mosaic_scale, cfg.mosaic_center, cfg.mosaic_min_visible, cfg.mosaic_fill, cfg.mixup_alpha) == \
        (0.0, 0.0, (0.5, 1.5), 0.25, 0.25, 114.0, 1.5)
    assert not cfg.compose and not A.AugmentConfig(None).compose
    cfg = A.AugmentConfig(config(mosaic=0.5, mosaic_scale='0.4, 1.2', mosaic_center=0.3, mosaic_min_visible=0.1, mosaic_fill=0, mixup=1, mixup_alpha=8))
    assert (cfg.mosaic, cfg.mixup, cfg.mosaic_scale, cfg.mosaic_center, cfg.mosaic_min_visible, cfg.mosaic_fill, cfg.mixup_alpha) == \
        (0.5, 1.0, (0.4, 1.2), 0.3, 0.1, 0.0, 8.0)
    assert cfg.compose and A.AugmentConfig(config(mixup=0.1)).compose and A.AugmentConfig(config(mosaic=0.1)).compose


@pytest.mark.parametrize('key, bad', [
    ('mosaic', '-0.1'), ('mosaic', '1.5'), ('mosaic', 'yes'), ('mosaic', 'nan'), ('mosaic', ''),
    ('mixup', '-1'), ('mixup', '2'), ('mixup', 'on'),
    ('mosaic_scale', '0.5'), ('mosaic_scale', '1.5 0.5'), ('mosaic_scale', '0 1'), ('mosaic_scale', '0.5 1 2'), ('mosaic_scale', 'a b'), ('mosaic_scale', '0.5 inf'),
    ('mosaic_center', '0.6'), ('mosaic_center', '-0.1'), ('mosaic_center', 'x'),
    ('mosaic_min_visible', '1.1'), ('mosaic_min_visible', '-0.5'),
    ('mosaic_fill', '256'), ('mosaic_fill', '-1'), ('mosaic_fill', 'grey'),
    ('mixup_alpha', '0'), ('mixup_alpha', '-2'), ('mixup_alpha', 'inf'),
])
def test_config_validation(key, bad):
    with pytest.raises(ValueError, match=r'\b%s\b' % key) as e:
        A.AugmentConfig(config(**{key: bad}))
    assert ('%s =' % key) in str(e.value)                         # (mosaic_scale's message does not pass for mosaic's)
