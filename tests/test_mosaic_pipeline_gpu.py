"""DeviceInputPipeline with `[mi355x] mosaic` / `mixup` (yolo_tf_amd/utils/augment.py) against the specification in tests/mosaic_ref.py: the
six label tensors bit for bit, the images at the project's bound for the per-pixel chain; the same seed twice; the keys absent against a
directly assembled yolo2_augment_images batch; and a size change in the middle of the stream."""
import configparser
import os

import numpy as np
import pytest
import torch

import augment_cases as C
import mosaic_ref as M
from oracle import yolo2_ref as R
from test_augment_gpu import run_augment

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = C.GPU_VS_ORACLE_TOL
B, CLASSES = 4, 20


@pytest.fixture(scope='module')
def ops():
    from yolo_tf_amd import ops as _ops
    _ops._lib.load()
    return _ops


def config(**keys):
    ini = configparser.ConfigParser()
    ini.read(os.path.join(ROOT, 'config.ini'))
    for k, v in keys.items():
        ini.set('mi355x', k, str(v))
    return ini


def dataset():
    rng = np.random.RandomState(12)
    images = [rng.randint(0, 256, (50 + 9 * i, 150 - 8 * i, 3)).astype(np.uint8) for i in range(10)]
    objects = []
    for im in images:
        h, w = im.shape[:2]
        k = rng.randint(1, 5)
        x0, y0 = rng.uniform(0, 0.6 * w, k), rng.uniform(0, 0.6 * h, k)
        objects.append((rng.randint(0, CLASSES, k).astype(np.int32), np.stack([x0, y0, x0 + rng.uniform(4, 0.39 * w, k), y0 + rng.uniform(4, 0.39 * h, k)], 1).astype(np.float32)))
    return images, objects


class Labels(object):
    """What the pipeline needs of a TrainSession: the six label tensors (dirty) and the current size."""

    def __init__(self, cw, ch, size):
        cells = cw * ch
        shapes = [(B, cells, 1), (B, cells, 1, CLASSES), (B, cells, 1, 4), (B, cells, 1, 2), (B, cells, 1, 2), (B, cells, 1)]
        self.labels = [torch.full(s, 5.0, dtype=torch.float32, device='cuda') for s in shapes]
        self.size = size


def check_against_the_specification(ops, got, labels, spec_images, images, W, H, cw, ch, fill):
    for b, im in enumerate(spec_images):
        want = R.transform_labels(im['classes'], im['boxes'], CLASSES, cw, ch)
        for o, r in zip(labels, want):
            np.testing.assert_array_equal(o[b].cpu().numpy().reshape(r.shape), r)
        photo = dict(im['photo'])
        if photo['noise_scale'] is not None:
            flat = np.full((H, W, 3), 128, np.uint8)
            photo['noise'] = run_augment(ops, [flat], [dict(noise_scale=photo['noise_scale'], noise_seed=photo['noise_seed'])], W, H)[0] - np.float32(128)
        layers = [[dict(t, src=images[t['index']]) for t in layer] for layer in im['layers']]
        err = np.abs(got[b] - M.compose(layers, photo, im['lam'], fill, W, H)).max()
        assert err <= TOL, 'image %d: %.3e' % (b, err)


def test_pipeline_against_the_specification(ops):
    from yolo_tf_amd.utils import augment as A
    images, objects = dataset()
    W, H, cw, ch = 96, 64, 3, 2
    ini = config(mosaic=1, mixup=0.5)
    sizes = [(im.shape[1], im.shape[0]) for im in images]
    runs = []
    for _ in range(2):                                                        # the same seed twice
        pipe = A.DeviceInputPipeline(images, objects, B, W, H, CLASSES, cw, ch, config=ini, seed=3)
        assert pipe.cfg.compose
        session, batches = Labels(cw, ch, (W, H)), []
        for _ in range(2):
            out = pipe.next(session).cpu().numpy()
            pipe.check()                                                      # a mosaic never raises transform_labels' flag
            batches.append((out, [t.clone() for t in session.labels]))
        runs.append(batches)
    for (a, la), (b, lb) in zip(*runs):
        np.testing.assert_array_equal(a, b)
        assert all(torch.equal(x, y) for x, y in zip(la, lb))
    rng = np.random.RandomState(3)
    cfg = A.AugmentConfig(ini)
    mixed = mosaics = 0
    for out, labels in runs[0]:
        idx = rng.randint(0, len(images), B)
        spec = [M.draw_image(cfg, rng, int(i), sizes, objects, W, H) for i in idx]
        mixed += sum(len(im['layers']) == 2 for im in spec)
        mosaics += sum(len(layer) == 4 for im in spec for layer in im['layers'])
        assert out.shape == (B, H, W, 3) and out.min() >= 0 and out.max() <= 255
        check_against_the_specification(ops, out, labels, spec, images, W, H, cw, ch, cfg.mosaic_fill)
    assert 0 < mixed < 2 * B and mosaics == 2 * B + mixed


def test_off_equals_parent(ops):
    """The keys absent: the batch is the one a directly assembled yolo2_augment_images launch gives for `draw`'s decisions, bit for bit
    (tests/test_mosaic_cpu.py holds `draw` and the stream to the parent's), and so are the labels."""
    from yolo_tf_amd._lib import AugmentParams
    from yolo_tf_amd.utils import augment as A
    from yolo_tf_amd.utils import data
    images, objects = dataset()
    W, H, cw, ch = 96, 64, 3, 2
    ini = config()
    pipe = A.DeviceInputPipeline(images, objects, B, W, H, CLASSES, cw, ch, config=ini, seed=5)
    assert not pipe.cfg.compose
    session = Labels(cw, ch, (W, H))
    rng, cfg = np.random.RandomState(5), A.AugmentConfig(ini)
    offsets = np.cumsum([0] + [im.size for im in images])[:-1]
    for _ in range(2):
        got = pipe.next(session).cpu().numpy()
        pipe.check()
        idx = rng.randint(0, len(images), B)
        arr = (AugmentParams * B)()
        for b, (d, i) in enumerate(zip(arr, idx)):
            p, boxes = A.draw(cfg, rng, (images[i].shape[1], images[i].shape[0]), objects[i][1], W, H)
            d.src_offset, d.src_w, d.src_h = int(offsets[i]), images[i].shape[1], images[i].shape[0]
            d.crop_x, d.crop_y, d.crop_w, d.crop_h = p['crop']
            d.flags = p['flags']
            d.brightness, d.saturation, d.hue, d.contrast = p['brightness'], p['saturation'], p['hue'], p['contrast']
            d.noise_scale, d.noise_seed = p['noise_scale'], p['noise_seed'] & (2 ** 64 - 1)
            for o, r in zip(session.labels, data.transform_labels(objects[i][0], boxes, CLASSES, cw, ch)):
                np.testing.assert_array_equal(o[b].cpu().numpy().reshape(r.shape), r)
        out = torch.full((B, H, W, 3), -1.0, dtype=torch.float32, device='cuda')
        ops.augment_images(pipe.src, torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda(), pipe.ws, out, B, H, W,
                           any(a.flags & A.CONTRAST for a in arr))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got, out.cpu().numpy())
    assert all(np.array_equal(x, y) for x, y in zip(pipe.rng.get_state()[1:], rng.get_state()[1:]))


def test_multiscale(ops):
    """After set_size the frame and the grid follow, and the draws are those the other size would have seen: two pipelines with one
    seed, one of which changes to 64 x 64 after its first batch."""
    from yolo_tf_amd.utils import augment as A
    images, objects = dataset()
    ini = config(mosaic=0.7, mixup=0.5)
    sizes = [(im.shape[1], im.shape[0]) for im in images]
    make = lambda: A.DeviceInputPipeline(images, objects, B, 96, 96, CLASSES, 3, 3, config=ini, seed=9, sizes=[(64, 64), (96, 96)], downsampling=(32, 32))
    changing, staying = make(), make()
    large, small = Labels(3, 3, (96, 96)), Labels(2, 2, (64, 64))
    first = changing.next(large)
    assert first.shape == (B, 96, 96, 3)
    np.testing.assert_array_equal(first.cpu().numpy(), staying.next(large).cpu().numpy())
    out = changing.next(small)
    changing.check()
    assert out.shape == (B, 64, 64, 3) and out.is_contiguous() and (changing.W, changing.H, changing.cell_width, changing.cell_height) == (64, 64, 2, 2)
    got = out.cpu().numpy()
    other, _, _, _ = staying.assemble(staying.sample())                       # the same draws at 96 x 96
    rng, cfg = np.random.RandomState(9), A.AugmentConfig(ini)
    for W in (96, 64):
        idx = rng.randint(0, len(images), B)
        spec = [M.draw_image(cfg, rng, int(i), sizes, objects, W, W) for i in idx]
    for im, at96 in zip(spec, other.images):
        assert im['lam'] == at96['lam'] and im['centers'] == [l['center'] for l in at96['layers']]
        assert [[(t['index'], t['crop'], t['flip']) for t in l] for l in im['layers']] == [[(t['index'], t['crop'], t['flip']) for t in l['tiles']] for l in at96['layers']]
    check_against_the_specification(ops, got, small.labels, spec, images, 64, 64, 2, 2, cfg.mosaic_fill)
    assert all(np.array_equal(x, y) for x, y in zip(changing.rng.get_state()[1:], staying.rng.get_state()[1:]))
