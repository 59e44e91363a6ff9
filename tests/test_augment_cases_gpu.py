"""yolo2_augment_images and yolo2_transform_labels (csrc/augment.hip) on the cases of tests/augment_cases.py; what each case reaches, and the
tolerance against the float64 reference, is established without a GPU in tests/test_augment_cases_cpu.py.

Every image case is held to the oracle at the project's 2e-3 (0..255 scale) and to the independent float64 reference (tests/augment_ref.py)
at ORACLE_VS_F64_TOL + 2e-3; the copy-shortcut and integer-downscale cases, flipped or not, to the source bytes bit for bit.  Every image
of a batch case must equal the same image launched alone, bit for bit; the source offset beyond 2^32 is checked with decoys at the offsets a
truncated or sign-extended offset would read.  The label cases are bit-exact against the host port and within tests/augment_cases.py's
label_tolerances of the float64 reference.  The last test drives DeviceInputPipeline.assemble + launch end to end.

Not tested, on purpose: the per-channel mean behind the contrast op is summed with f64 atomics in whatever order the waves arrive, so a
contrast image is not bitwise reproducible between launches in principle (in f64 the spread is far below an f32 ulp of the mean, so it
hardly ever shows).  Contrast images are therefore compared at 2e-3 where the others are compared bit for bit, and no test asks for a
run-to-run equality that could only sometimes fail."""
import configparser
import os

import numpy as np
import pytest
import torch

import augment_cases as C
from oracle import yolo2_ref as R
from test_augment_gpu import _device_labels, run_augment

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = C.GPU_VS_ORACLE_TOL
TOL_F64 = C.ORACLE_VS_F64_TOL + C.GPU_VS_ORACLE_TOL


@pytest.fixture(scope='module')
def ops():
    from yolo_tf_amd import ops as _ops
    _ops._lib.load()
    return _ops


def device_noise(ops, scale, seed, W, H):
    """The kernel's own noise for (seed, H x W), read back through a flat source of 128 of the output's size (the copy shortcut; 128 +- 2
    scale stays inside the clip).  128 + n rounds to f32 at that magnitude, so n is known to 2^-17 = 8e-6, far inside every tolerance."""
    flat = np.full((H, W, 3), 128, np.uint8)
    return run_augment(ops, [flat], [dict(noise_scale=scale, noise_seed=seed)], W, H)[0] - np.float32(128)


def check_image(got, c, noise=None):
    """One device image against both references, every pixel."""
    if noise is None and c['name'] in C.IMAGES:
        ref, f64 = C.oracle(c['name']), C.f64(c['name'])                              # computed once per session
    else:
        ref, f64 = C.oracle_of(c, noise), C.f64_of(c, noise)
    assert got.shape == ref.shape and got.min() >= 0 and got.max() <= 255
    err, err64 = np.abs(got - ref), np.abs(got - f64)
    print('%s: %.3e vs the oracle, %.3e vs float64' % (c['name'], err.max(), err64.max()))
    assert err.max() <= TOL, '%s: %.3e vs the oracle at %s' % (c['name'], err.max(), np.unravel_index(err.argmax(), err.shape))
    assert err64.max() <= TOL_F64, '%s: %.3e vs float64 at %s' % (c['name'], err64.max(), np.unravel_index(err64.argmax(), err64.shape))


@pytest.mark.parametrize('name', C.NAMES)
def test_image_case(ops, name):
    c = C.case(name)
    got = run_augment(ops, [c['src']], [c['p']], c['W'], c['H'])[0]
    noise = None
    if c['p'].get('noise_scale') is not None:
        noise = device_noise(ops, c['p']['noise_scale'], c['p']['noise_seed'], c['W'], c['H'])
        assert np.abs(noise).max() <= 2 * c['p']['noise_scale'] + 1e-4 and noise.std() > 0.5 * c['p']['noise_scale']
    check_image(got, c, noise)
    if {'copy', 'int_down'} & c['tags']:
        np.testing.assert_array_equal(got, C.exact_expectation(c))                    # exact arithmetic: the source bytes
    if 'clamp' in c['tags']:
        assert not got.any()                                                          # one tap beyond the crop reads 255
    if 'grey' in c['tags']:
        assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 1], got[..., 2])


@pytest.mark.parametrize('name', C.BATCHES)
def test_batch_case(ops, name):
    b = C.batch(name)
    src = torch.from_numpy(np.concatenate([s.reshape(-1) for s in b['sources']])).cuda()
    got = run_augment(ops, [b['sources'][k] for k, _ in b['items']], [p for _, p in b['items']], b['W'], b['H'],
                      offsets=[b['offsets'][k] for k, _ in b['items']], src=src)        # the workspace holds garbage beforehand
    for i, (k, p) in enumerate(b['items']):
        c = C.batch_image(name, i)
        check_image(got[i], c)
        alone = run_augment(ops, [b['sources'][k]], [p], b['W'], b['H'])[0]
        if p.get('contrast') is None:
            np.testing.assert_array_equal(got[i], alone, err_msg=c['name'])
        else:                                                                         # f64 atomics in launch order behind the mean
            assert np.abs(got[i] - alone).max() <= TOL, c['name']


def test_source_offset_beyond_32_bits(ops):
    """The image sits at 2^32 + 4096 of an uninitialised buffer of 2^32 + 64 KiB; different images sit at 4096 (what the low 32 bits of the
    offset address) and at 2^31 + 4096.  Every address a wrong offset arithmetic of that kind would form lies inside the allocation."""
    rng = np.random.RandomState(32)
    image, decoy_lo, decoy_mid = [rng.randint(0, 256, (30, 40, 3)).astype(np.uint8) for _ in range(3)]
    total, at = 2 ** 32 + 64 * 1024, 2 ** 32 + 4096
    assert at + image.size <= total
    buf = torch.empty(total, dtype=torch.uint8, device='cuda')
    try:
        for off, im in ((4096, decoy_lo), (2 ** 31 + 4096, decoy_mid), (at, image)):
            buf[off:off + im.size] = torch.from_numpy(im.reshape(-1)).cuda()
        p = dict(flip=True, saturation=1.2)
        got = run_augment(ops, [image], [p], 53, 41, offsets=[at], src=buf)[0]
    finally:
        del buf
        torch.cuda.empty_cache()
    c = {'name': 'offset_2^32+4096', 'src': image, 'W': 53, 'H': 41, 'p': p, 'tags': frozenset()}
    check_image(got, c)
    for decoy in (decoy_lo, decoy_mid):
        assert np.abs(got - R.augment_image(decoy, p, 53, 41)).max() > 50             # and the decoys are told apart


def test_noise_seeds_and_slots(ops):
    flat = np.full((1, 257, 3), 128, np.uint8)                                        # H * W = 257: a ragged last wave
    src = torch.from_numpy(flat.reshape(-1)).cuda()
    seeds = (123456789012345, 123456789012345, 123456789012346)
    got = run_augment(ops, [flat] * 3, [dict(noise_scale=10.0, noise_seed=s) for s in seeds], 257, 1, offsets=[0, 0, 0], src=src) - np.float32(128)
    np.testing.assert_array_equal(got[0], got[1])                                     # the slot does not enter the counter
    assert np.abs(got[0] - got[2]).max() > 1.0 and (got[0] != got[2]).mean() > 0.99
    assert np.abs(got).max() <= 20.0 + 1e-4 and 7.0 < got.std() < 10.5                # sigma of N(0, 1) cut at 2: 0.88


@pytest.mark.parametrize('level', [0, 255])
def test_noise_is_added_before_grey_and_before_the_clip(ops, level):
    W = H = 64
    flat = np.full((H, W, 3), level, np.uint8)
    noise = device_noise(ops, 10.0, 99, W, H)
    got = run_augment(ops, [flat, flat], [dict(noise_scale=10.0, noise_seed=99), dict(noise_scale=10.0, noise_seed=99, gray=True)], W, H)
    assert got.min() >= 0 and got.max() <= 255
    for g in got:
        assert 0.45 < (g == level).mean() < 0.55                                      # half of the noise points out of range and is clipped
    np.testing.assert_allclose(got[0], np.clip(level + noise.astype(np.float64), 0, 255), atol=1e-4)
    grey = noise.astype(np.float64) @ [0.2989, 0.5870, 0.1140] + level * (0.2989 + 0.5870 + 0.1140)
    np.testing.assert_allclose(got[1], np.clip(grey, 0, 255)[..., None].repeat(3, -1), atol=1e-3)       # the grey of the noisy pixel, then the clip
    assert np.array_equal(got[1][..., 0], got[1][..., 1]) and np.array_equal(got[1][..., 1], got[1][..., 2])


@pytest.mark.parametrize('name', C.LABELS)
def test_label_case(ops, name):
    from yolo_tf_amd.utils import data
    L = C.labels(name)
    outs, err = _device_labels(ops, L['objs'], L['classes'], L['cw'], L['ch'])        # outputs pre-filled with 5.0, the flag starts at 0
    assert err == L['err']
    for b, (cls, box) in enumerate(L['objs']):
        got = [o[b] for o in outs]
        C.assert_labels_match_f64(got, name, b)
        if C.labels_f64(name)[b][0][6]:
            continue                                                                  # the host port raises for this image, as the reference does
        for g, r in zip(got, data.transform_labels(cls, box, L['classes'], L['cw'], L['ch'])):
            np.testing.assert_array_equal(g.reshape(r.shape), r, err_msg='%s[%d]' % (name, b))


def test_pipeline_end_to_end(ops):
    """DeviceInputPipeline.assemble + launch, three batches of 8 at 96 x 64 on a 3 x 2 grid from 12 images of different sizes: every image
    is the oracle's for its own draw (noise taken out by launching the same parameters again with the flag cleared), the six label
    tensors are the host port's for the boxes assemble returned."""
    from yolo_tf_amd.utils import augment as A
    from yolo_tf_amd.utils import data
    ini = configparser.ConfigParser()
    ini.read(os.path.join(ROOT, 'config.ini'))
    rng = np.random.RandomState(12)
    images = [rng.randint(0, 256, (50 + 9 * i, 150 - 8 * i, 3)).astype(np.uint8) for i in range(12)]
    objects = []
    for im in images:
        h, w = im.shape[:2]
        k = rng.randint(1, 5)
        x0, y0 = rng.uniform(0, 0.6 * w, k), rng.uniform(0, 0.6 * h, k)
        objects.append((rng.randint(0, 20, k), np.stack([x0, y0, x0 + rng.uniform(4, 0.39 * w, k), y0 + rng.uniform(4, 0.39 * h, k)], 1)))
    B, W, H, classes, cw, ch = 8, 96, 64, 20, 3, 2
    pipe = A.DeviceInputPipeline(images, objects, B, W, H, classes, cw, ch, config=ini, seed=3)
    cells = cw * ch
    shapes = [(B, cells, 1), (B, cells, 1, classes), (B, cells, 1, 4), (B, cells, 1, 2), (B, cells, 1, 2), (B, cells, 1)]
    flags_seen = 0
    for _ in range(3):
        idx = pipe.sample()
        arr, cls, box, first = pipe.assemble(idx)
        labels = [torch.full(s, 5.0, dtype=torch.float32, device='cuda') for s in shapes]
        noisy = pipe.launch(arr, cls, box, first, labels).cpu().numpy()
        pipe.check()
        for a in arr:
            flags_seen |= a.flags
            a.flags &= ~A.NOISE
        clean = pipe.launch(arr, cls, box, first, labels).cpu().numpy()
        pipe.check()
        assert noisy.min() >= 0 and noisy.max() <= 255
        for i, a in enumerate(arr):
            p = dict(crop=(a.crop_x, a.crop_y, a.crop_w, a.crop_h), flip=bool(a.flags & A.FLIP), gray=bool(a.flags & A.GRAY))
            for key, bit in (('brightness', A.BRIGHTNESS), ('saturation', A.SATURATION), ('hue', A.HUE), ('contrast', A.CONTRAST)):
                p[key] = getattr(a, key) if a.flags & bit else None
            err = np.abs(clean[i] - R.augment_image(images[idx[i]], p, W, H)).max()
            assert err <= TOL, 'image %d (source %d, %s): %.3e' % (i, idx[i], p, err)
            for o, r in zip(labels, data.transform_labels(cls[first[i]:first[i + 1]], box[first[i]:first[i + 1]], classes, cw, ch)):
                np.testing.assert_array_equal(o[i].cpu().numpy().reshape(r.shape), r)
    assert flags_seen & A.NOISE and flags_seen & A.FLIP and flags_seen & A.CONTRAST   # the draws did take these branches
