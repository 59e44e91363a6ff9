"""yolo2_compose_images (csrc/compose.hip) through the C ABI.  Where both sides are the device's own arithmetic -- one tile against
yolo2_augment_images, a tile's window against that entry's output at the view's size, the blend against the two layers' own outputs -- the
comparison is bit for bit; the photometric chain on a composite is held to tests/mosaic_ref.py's `compose` at the bound the project
already has for this per-pixel chain, augment_cases.GPU_VS_ORACLE_TOL.

Contrast: the f64 channel sums behind the mean are added with atomics in the order the waves arrive (tests/test_augment_cases_gpu.py), so a
contrast image is bitwise reproducible only as long as no such reordering moves the f32 mean; both entries add the same per-wave partial
sums, and the comparisons here are bit for bit as specified."""
import numpy as np
import pytest
import torch

import augment_cases as C
import mosaic_ref as M
from test_augment_gpu import run_augment

pytestmark = pytest.mark.gpu
TOL = C.GPU_VS_ORACLE_TOL
FILL = 114.0


@pytest.fixture(scope='module')
def ops():
    from yolo_tf_amd import ops as _ops
    _ops._lib.load()
    return _ops


def full_tile(k, W, H, crop=None, flip=False):
    return dict(k=k, crop=crop, view=(W, H), origin=(0, 0), rect=(0, 0, W, H), flip=flip)


def pack(sources):
    offsets = [int(v) for v in np.cumsum([0] + [s.size for s in sources])[:-1]]
    return torch.from_numpy(np.concatenate([np.ascontiguousarray(s).reshape(-1) for s in sources])).cuda(), offsets


def run_compose(ops, sources, images, W, H, L=1, T=1, fill=FILL, src=None, offsets=None, dirty=9.0, mix_none=False):
    """One launch.  sources: uint8 images (packed back to back unless `src` / `offsets` place them); images: per output image
    dict(layers=[[tile, ...], ...], photo=dict as run_augment reads it, mix=weight of layer 0).  A tile is dict(k = source index, crop,
    view, origin, rect, flip); slots a layer does not list stay empty.  `ws` and `out` hold `dirty` beforehand."""
    from yolo_tf_amd._lib import AugmentParams, ComposeTile
    from yolo_tf_amd.utils import augment as A
    B = len(images)
    if src is None:
        src, offsets = pack(sources)
    tiles, photo, mix = (ComposeTile * (B * L * T))(), (AugmentParams * B)(), np.ones(B, np.float32)
    for b, im in enumerate(images):
        for l, layer in enumerate(im['layers']):
            for k, t in enumerate(layer):
                d, s = tiles[(b * L + l) * T + k], sources[t['k']]
                d.src_offset, d.src_w, d.src_h = offsets[t['k']], s.shape[1], s.shape[0]
                d.crop_x, d.crop_y, d.crop_w, d.crop_h = t.get('crop') or (0, 0, s.shape[1], s.shape[0])
                d.view_w, d.view_h = t['view']
                d.origin_x, d.origin_y = t['origin']
                d.x0, d.y0, d.x1, d.y1 = t['rect']
                d.flip = int(bool(t.get('flip')))
        p, d, fl = im.get('photo') or {}, photo[b], 0
        if p.get('gray'):
            fl |= A.GRAY
        for key, bit in (('brightness', A.BRIGHTNESS), ('saturation', A.SATURATION), ('hue', A.HUE), ('contrast', A.CONTRAST)):
            if p.get(key) is not None:
                fl |= bit
                setattr(d, key, p[key])
        if p.get('noise_scale') is not None:
            fl |= A.NOISE
            d.noise_scale, d.noise_seed = p['noise_scale'], p.get('noise_seed', 7)
        d.flags = fl | A.FLIP                                             # the geometry fields of `photo` and its FLIP are ignored
        d.crop_w = d.crop_h = d.src_w = d.src_h = -12345
        mix[b] = im.get('mix', 1.0)
    up = lambda a: torch.frombuffer(bytearray(bytes(a)), dtype=torch.uint8).cuda()
    ws = torch.full((3 * B,), dirty, dtype=torch.float64, device='cuda')
    out = torch.full((B, H, W, 3), dirty, dtype=torch.float32, device='cuda')
    ops.compose_images(src, up(tiles), up(photo), None if mix_none else torch.from_numpy(mix).cuda(), ws, out, B, L, T, H, W, fill,
                       any(a.flags & A.CONTRAST for a in photo))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def photo_of(p):
    return {k: v for k, v in p.items() if k not in ('crop', 'flip')}


# ---- one tile equals the old entry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', C.NAMES)
def test_one_tile_equals_augment_images(ops, name):
    c = C.case(name)
    want = run_augment(ops, [c['src']], [c['p']], c['W'], c['H'])[0]
    tile = full_tile(0, c['W'], c['H'], c['p'].get('crop'), c['p'].get('flip'))
    got = run_compose(ops, [c['src']], [dict(layers=[[tile]], photo=photo_of(c['p']))], c['W'], c['H'])[0]
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize('name', C.BATCHES)
def test_one_tile_equals_augment_images_batch(ops, name):
    b = C.batch(name)
    src, _ = pack(b['sources'])
    want = run_augment(ops, [b['sources'][k] for k, _ in b['items']], [p for _, p in b['items']], b['W'], b['H'],
                       offsets=[b['offsets'][k] for k, _ in b['items']], src=src)
    images = [dict(layers=[[full_tile(k, b['W'], b['H'], p.get('crop'), p.get('flip'))]], photo=photo_of(p)) for k, p in b['items']]
    got = run_compose(ops, b['sources'], images, b['W'], b['H'], src=src, offsets=b['offsets'])
    np.testing.assert_array_equal(got, want)
    if name == 'b8':                                                          # unused slots and an unread second layer change nothing
        np.testing.assert_array_equal(run_compose(ops, b['sources'], images, b['W'], b['H'], L=2, T=4, src=src, offsets=b['offsets']), want)


@pytest.mark.parametrize('B', [1, 9, 64])
def test_one_tile_equals_augment_images_grids(ops, B):
    """8 x 8 frames at the three batch sizes at which the launcher picks another grid (128, 32 and 8 workgroups per image)."""
    rng = np.random.RandomState(B)
    sources = [rng.randint(0, 256, (11 + i % 5, 9 + i % 7, 3)).astype(np.uint8) for i in range(B)]
    colour = (dict(), dict(flip=True, hue=0.02), dict(contrast=1.3, saturation=0.8), dict(noise_scale=9.0, noise_seed=5, gray=True), dict(brightness=-20.0, crop=(1, 2, 6, 7)))
    params = [colour[i % len(colour)] for i in range(B)]
    want = run_augment(ops, sources, params, 8, 8)
    images = [dict(layers=[[full_tile(i, 8, 8, p.get('crop'), p.get('flip'))]], photo=photo_of(p)) for i, p in enumerate(params)]
    np.testing.assert_array_equal(run_compose(ops, sources, images, 8, 8), want)


# ---- windows ----------------------------------------------------------------------------------------------------------------------------
W, H = 61, 47
_rng = np.random.RandomState(2024)
SOURCES = [_rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((40, 55), (70, 33), (52, 52), (90, 120))]
SOURCES.append(np.full((30, 30, 3), 255, np.uint8))                           # the poison of the blend test: inside the buffer


def mosaic(cx, cy, views, crops=(None,) * 4, flips=(False, True, False, True), sources=(0, 1, 2, 3), skip=()):
    rects = [(0, 0, cx, cy), (cx, 0, W, cy), (0, cy, cx, H), (cx, cy, W, H)]
    return [dict(k=sources[q], crop=crops[q], view=views[q], origin=M.origin(q, cx, cy, *views[q]), rect=rects[q], flip=flips[q])
            for q in range(4) if q not in skip]


LAYOUTS = {
    'centre_interior': mosaic(30, 20, [(40, 30), (45, 37), (38, 41), (50, 33)]),
    'cx_1': mosaic(1, 20, [(40, 30), (70, 37), (38, 41), (66, 33)]),
    'cx_W_minus_1': mosaic(W - 1, 20, [(70, 30), (45, 37), (64, 41), (50, 33)]),
    'cy_1': mosaic(30, 1, [(40, 30), (45, 37), (38, 50), (50, 52)]),
    'views_larger_than_quadrants': mosaic(30, 20, [(80, 60), (75, 70), (90, 41), (91, 66)]),            # negative origins
    'views_smaller_than_quadrants': mosaic(30, 20, [(12, 9), (20, 11), (7, 19), (25, 20)]),             # fill shows
    'view_w_1': mosaic(30, 20, [(1, 30), (1, 37), (1, 1), (50, 1)]),
    'crop_equals_view': mosaic(30, 20, [(40, 30), (33, 37), (38, 41), (50, 33)], crops=((5, 3, 40, 30), (0, 10, 33, 37), (9, 8, 38, 41), (60, 50, 50, 33))),
    'cropped': mosaic(33, 25, [(40, 30), (45, 37), (38, 41), (50, 33)], crops=((5, 3, 31, 17), (2, 10, 30, 55), (9, 8, 1, 41), (60, 50, 13, 1))),
    'three_tiles_of_four_slots': mosaic(30, 20, [(40, 30), (45, 37), (38, 41), (50, 33)], skip=(2,)),
}


def expected_layer(ops, tiles, untouched):
    """A layer without colour from yolo2_augment_images outputs at each view's size; `untouched` where no tile's rectangle reaches."""
    out = np.full((H, W, 3), np.float32(untouched), np.float32)
    for t in tiles:
        vw, vh = t['view']
        view = run_augment(ops, [SOURCES[t['k']]], [dict(crop=t['crop'], flip=t['flip'])], vw, vh)[0]
        x0, y0, x1, y1 = t['rect']
        out[y0:y1, x0:x1] = np.float32(FILL)
        ox, oy = t['origin']
        ax0, ay0, ax1, ay1 = max(x0, ox), max(y0, oy), min(x1, ox + vw), min(y1, oy + vh)
        if ax1 > ax0 and ay1 > ay0:
            out[ay0:ay1, ax0:ax1] = view[ay0 - oy:ay1 - oy, ax0 - ox:ax1 - ox]
    return out


@pytest.mark.parametrize('name', sorted(LAYOUTS))
def test_windows(ops, name):
    tiles = LAYOUTS[name]
    got = run_compose(ops, SOURCES, [dict(layers=[tiles])], W, H, T=4, dirty=-3.0)[0]
    want = expected_layer(ops, tiles, untouched=-3.0)            # (the unused slot's quadrant is nobody's: not written)
    np.testing.assert_array_equal(got, want)
    if name == 'views_smaller_than_quadrants':
        assert (got == FILL).all(-1).mean() > 0.5
    spec = M.layer_image([dict(t, src=SOURCES[t['k']]) for t in tiles], FILL, W, H)
    covered = got[..., 0] != -3.0
    assert np.abs(got - spec)[covered].max() <= TOL


# ---- blend ------------------------------------------------------------------------------------------------------------------------------
LAYER_A, LAYER_B = LAYOUTS['centre_interior'], mosaic(41, 9, [(30, 30), (25, 47), (58, 41), (15, 33)], sources=(3, 2, 1, 0), flips=(True, True, False, False))


@pytest.mark.parametrize('lam', [0.5, 0.3, float(np.float32(np.random.RandomState(6).beta(1.5, 1.5)))])
def test_blend(ops, lam):
    a = run_compose(ops, SOURCES, [dict(layers=[LAYER_A])], W, H, T=4)[0]
    b = run_compose(ops, SOURCES, [dict(layers=[LAYER_B])], W, H, T=4)[0]
    got = run_compose(ops, SOURCES, [dict(layers=[LAYER_A, LAYER_B], mix=lam)], W, H, L=2, T=4)[0]
    lam = np.float32(lam)
    np.testing.assert_array_equal(got, a * lam + b * (np.float32(1) - lam))
    assert 0 < lam < 1 and np.abs(got - a).max() > 10 and np.abs(got - b).max() > 10


def test_mix_one_reads_layer_0_only(ops):
    """mix == 1: layer 0 bit for bit, although layer 1's tiles point at a source of 255s (inside the buffer) that would show if read; the
    second image of the batch, with mix 0.5, does show it."""
    a = run_compose(ops, SOURCES, [dict(layers=[LAYER_A])], W, H, T=4)[0]
    poison = [dict(t, k=4, crop=None) for t in LAYER_B]
    got = run_compose(ops, SOURCES, [dict(layers=[LAYER_A, poison], mix=1.0), dict(layers=[LAYER_A, poison], mix=0.5)], W, H, L=2, T=4)
    np.testing.assert_array_equal(got[0], a)
    assert (got[1] != a).mean() > 0.5
    single = run_compose(ops, SOURCES, [dict(layers=[LAYER_A])], W, H, L=1, T=4, mix_none=True)[0]      # L = 1: `mix` may be NULL
    np.testing.assert_array_equal(single, a)


# ---- colour on the composite ------------------------------------------------------------------------------------------------------------
def device_noise(ops, scale, seed):
    flat = np.full((H, W, 3), 128, np.uint8)
    return run_augment(ops, [flat], [dict(noise_scale=scale, noise_seed=seed)], W, H)[0] - np.float32(128)


COLOUR = {
    'contrast_with_fill_visible': (['views_smaller_than_quadrants'], 1.0, dict(contrast=1.4)),
    'contrast_with_mixup': ([LAYER_A, LAYER_B], 0.35, dict(contrast=0.6)),
    'every_branch': ([LAYER_A, 'views_smaller_than_quadrants'], 0.62, dict(brightness=21.0, saturation=1.3, hue=-0.02, contrast=1.2, noise_scale=8.0, noise_seed=31)),
    'every_branch_grey': ([LAYER_B, LAYER_A], 0.45, dict(brightness=-30.0, saturation=0.7, hue=0.03, contrast=0.8, noise_scale=12.0, noise_seed=32, gray=True)),
    'saturation_hue_on_fill': (['views_smaller_than_quadrants'], 1.0, dict(saturation=1.5, hue=0.032)),
}


@pytest.mark.parametrize('name', sorted(COLOUR))
def test_colour_on_the_composite(ops, name):
    layers, lam, p = COLOUR[name]
    layers = [LAYOUTS[l] if isinstance(l, str) else l for l in layers]
    got = run_compose(ops, SOURCES, [dict(layers=layers, mix=lam, photo=p)], W, H, L=len(layers), T=4)[0]
    ref_p = dict(p)
    if p.get('noise_scale') is not None:
        ref_p['noise'] = device_noise(ops, p['noise_scale'], p['noise_seed'])
    want = M.compose([[dict(t, src=SOURCES[t['k']]) for t in l] for l in layers], ref_p, lam, FILL, W, H)
    err = np.abs(got - want)
    print('%s: %.3e vs the specification' % (name, err.max()))
    assert got.min() >= 0 and got.max() <= 255
    assert err.max() <= TOL, '%s: %.3e at %s' % (name, err.max(), np.unravel_index(err.argmax(), err.shape))
    if p.get('gray'):
        assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 1], got[..., 2])


def test_noise(ops):
    p = dict(noise_scale=10.0, noise_seed=123456789012345)
    a = run_compose(ops, SOURCES, [dict(layers=[LAYER_A], photo=p)], W, H, T=4)[0]
    b = run_compose(ops, SOURCES, [dict(layers=[LAYER_A], photo=p)], W, H, T=4)[0]
    clean = run_compose(ops, SOURCES, [dict(layers=[LAYER_A])], W, H, T=4)[0]
    np.testing.assert_array_equal(a, b)
    assert (a != clean).mean() > 0.9
    # the noise is indexed by the OUTPUT pixel: the field of yolo2_augment_images for the same seed and frame
    inside = (clean > 25) & (clean < 230)
    np.testing.assert_allclose((a - clean)[inside], device_noise(ops, 10.0, p['noise_seed'])[inside], atol=1e-4)


def test_dirty_buffers(ops):
    images = [dict(layers=[LAYER_A, LAYER_B], mix=0.4, photo=dict(contrast=1.3, hue=0.01)), dict(layers=[LAYER_B, LAYER_A], mix=1.0, photo=dict(saturation=1.2))]
    a = run_compose(ops, SOURCES, images, W, H, L=2, T=4, dirty=9.0)
    b = run_compose(ops, SOURCES, images, W, H, L=2, T=4, dirty=-1e30)
    c = run_compose(ops, SOURCES, images, W, H, L=2, T=4, dirty=float('nan'))
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, c)


# ---- arguments --------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(ops):
    from yolo_tf_amd._lib import HipKernelError
    image = [dict(layers=[LAYER_A], photo=dict(contrast=1.2))]
    with pytest.raises(HipKernelError, match='argument check failed'):
        run_compose(ops, SOURCES, image, W, H, L=3, T=4)
    with pytest.raises(HipKernelError, match='argument check failed'):
        run_compose(ops, SOURCES, image, W, H, L=1, T=5)
    with pytest.raises(HipKernelError, match='argument check failed'):
        run_compose(ops, SOURCES, image, W, H, L=2, T=4, mix_none=True)
    src, _ = pack(SOURCES)
    out = torch.full((1, H, W, 3), 7.0, dtype=torch.float32, device='cuda')
    junk = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    with pytest.raises(HipKernelError, match='argument check failed'):
        ops.compose_images(src, junk, junk, None, None, out, 1, 1, 4, H, W, FILL, True)       # contrast without a workspace
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                                                 # nothing was launched
