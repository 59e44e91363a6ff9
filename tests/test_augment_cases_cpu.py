"""The case table of the input pipeline (tests/augment_cases.py) checked without a GPU: the oracle against the independent float64 reference
(tests/augment_ref.py) on every pixel of every case, which is also where the tolerance of the GPU test is measured; each case shown to reach
what its id says; the hue == 1.0 sources found again by the bounded search; the host port of transform_labels against the float64 label
reference; and the image half tied to the box half: boxes painted into the source must land where augment.draw says they do."""
import configparser
import os

import numpy as np
import pytest

import augment_cases as C
import augment_ref as F
from oracle import yolo2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_is_complete_and_small():
    for g in C.GEOMETRY:
        assert 'geom_%s' % g in C.IMAGES and C.case('geom_%s_cropped' % g)['p']['crop'][:2] == (3, 2)
    assert sorted(c['H'] * c['W'] for c in map(C.case, ['geom_hw%d' % n for n in (1, 63, 65, 257, 32769)])) == [1, 63, 65, 257, 32769]
    for c in C.every_image():
        big = c['name'].startswith(('geom_hw257', 'geom_hw32769'))                   # 257 is prime, 32769 = 99 x 331: see the table's docstring
        assert max(c['src'].shape[:2]) <= 200 and (max(c['W'], c['H']) <= 150 or big), c['name']
    assert [len(C.batch(n)['items']) for n in ('b8', 'b64', 'b5_contrast_on_1_and_3')] == [8, 64, 5]
    assert [i for i, (_, p) in enumerate(C.batch('b5_contrast_on_1_and_3')['items']) if 'contrast' in p] == [1, 3]
    assert len(set(C.batch('shared_source')['offsets'])) == 1 and len(set(p['crop'] for _, p in C.batch('shared_source')['items'])) == 6
    a = C.batch('packed_first')['sources'][0]
    assert all(np.array_equal(C.batch(n)['sources'][k], a) for n, k in (('packed_middle', 1), ('packed_last', 2)))
    assert len({s.shape for s in C.batch('packed_first')['sources']}) == 3


# ---------------------------------------------------------------------------------------------------------------------
# the oracle against the float64 reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', C.NAMES)
def test_oracle_vs_f64(name):
    c = C.case(name)
    o, f = C.oracle(name), C.f64(name)
    assert o.shape == f.shape == (c['H'], c['W'], 3) and o.dtype == np.float32 and f.dtype == np.float64
    err = np.abs(o - f)                                                               # every pixel, every channel
    print('measured %s %.4e' % (name, err.max()))
    assert err.max() <= C.ORACLE_VS_F64_TOL, '%s: %.3e grey levels at %s' % (name, err.max(), np.unravel_index(err.argmax(), err.shape))


def test_oracle_vs_f64_measured_over_the_table():
    worst, pixels, where = 0.0, 0, None
    for c in C.every_image():
        err = float(np.abs(C.oracle_of(c) - C.f64_of(c)).max())
        pixels += c['H'] * c['W']
        if err > worst:
            worst, where = err, c['name']
    print('measured over %d pixels: %.4e grey levels (%s); ORACLE_VS_F64_MEASURED = %.4e' % (pixels, worst, where, C.ORACLE_VS_F64_MEASURED))
    assert worst <= C.ORACLE_VS_F64_TOL == 2 * C.ORACLE_VS_F64_MEASURED
    assert worst >= 0.5 * C.ORACLE_VS_F64_MEASURED, 'ORACLE_VS_F64_MEASURED is stale: measure it again'
    assert C.ORACLE_VS_F64_TOL < 1e-2                                                 # f32 rounding, not a difference of definitions


def test_f64_reference_known_answers():
    x = np.arange(8 * 6 * 3, dtype=np.float64).reshape(8, 6, 3)
    np.testing.assert_array_equal(F.resize(x, 4, 3), x[::2, ::2])
    assert F.resize(x, 8, 6) is x
    np.testing.assert_array_equal(F.resize(np.array([[0, 1], [2, 3]], float)[..., None].repeat(3, -1), 4, 4)[..., 0],
                                  [[0, .5, 1, 1], [1, 1.5, 2, 2], [2, 2.5, 3, 3], [2, 2.5, 3, 3]])
    h, s, v = F.to_hsv(np.array([[200., 10, 10], [10, 200, 10], [10, 10, 200], [200, 200, 10], [7, 7, 7], [0, 0, 0], [201, 100.99999, 101]]))
    np.testing.assert_allclose(h[:6], [0, 1 / 3, 2 / 3, 1 / 6, 0, 0], atol=1e-15)
    assert 1 - 1e-7 < h[6] < 1 and s[4] == 0 and s[5] == 0 and v[5] == 0
    # periodic: the hue just below 1 and the hue 0 give (almost) the same colour, the dominant channel stays
    np.testing.assert_allclose(F.saturation(np.array([[[201., np.nextafter(np.float32(101), 0), 101]]]), 1.2), [[[201, 81, 81]]], atol=1e-4)
    np.testing.assert_allclose(F.from_hsv(*F.to_hsv(x)), x, atol=1e-12)
    np.testing.assert_allclose(F.hue(np.array([[[200., 10, 10]]]), 1 / 3), [[[10, 200, 10]]], atol=1e-4)


# ---------------------------------------------------------------------------------------------------------------------
# each case reaches what its id says
# ---------------------------------------------------------------------------------------------------------------------
def _tagged(tag):
    names = [n for n in C.NAMES if tag in C.IMAGES[n][4]]
    assert names
    return names


@pytest.mark.parametrize('name', _tagged('clamp'))
def test_clamp_cases_tap_beyond_the_crop(name):
    c = C.case(name)
    x0, y0, cw, ch = c['p']['crop']
    h, w = c['src'].shape[:2]
    f = np.float32
    last_x = int(np.floor(f(c['W'] - 1) * (f(cw) / f(c['W'])))) + 1                   # the upper tap of the last column, before the clamp
    last_y = int(np.floor(f(c['H'] - 1) * (f(ch) / f(c['H'])))) + 1
    assert last_x > cw - 1 and last_y > ch - 1
    assert (c['src'][y0:y0 + ch, x0:x0 + cw] == 0).all() and int((c['src'] == 0).sum()) == 3 * cw * ch      # 255 everywhere else
    assert x0 + cw < w or y0 + ch < h or name in ('clamp_flush_both', 'clamp_last_pixel')               # the source goes on past the crop
    flush = {'clamp_flush_right': (True, False), 'clamp_flush_bottom': (False, True), 'clamp_flush_both': (True, True), 'clamp_last_pixel': (True, True)}.get(name)
    if flush:
        assert (x0 + cw == w, y0 + ch == h) == flush
    assert not C.oracle(name).any() and not C.f64(name).any()                        # a clamp at the source's edge would read 255


@pytest.mark.parametrize('name', _tagged('hue1'))
def test_hue1_cases_hold_a_hue_of_exactly_one(name):
    c = C.case(name)
    pre = C.before_hsv(c)
    hsv = R.rgb_to_hsv(pre)
    at = np.argwhere(hsv[..., 0] == np.float32(1))
    assert len(at), name
    y, x = at[0]
    r = pre[y, x, 0]
    assert r == pre[y, x].max() and r > 100
    # the periodic reference keeps the dominant channel, and so must the oracle: a literal HSVToRGB switch returns (m, m, m) here
    assert abs(C.f64(name)[y, x, 0] - r) < 1e-3 and abs(C.oracle(name)[y, x, 0] - r) < 1e-3


def test_hue1_search_finds_the_recorded_sources():
    found = C.search_hue1(**C.HUE1_SEARCH)
    assert found == [C.HUE1[k] for k in ('b', 'c', 'd')]
    assert C.HUE1_SEARCH['draws'] <= 5000 and all(max(f[1], f[2]) < 64 for f in found)
    assert len({f[0] for f in found} | {C.HUE1['a'][0]}) == 4 and len({f[1:3] for f in found} | {C.HUE1['a'][1:3]}) == 4


@pytest.mark.parametrize('name', _tagged('wrap'))
def test_wrap_cases_hold_hues_on_both_sides(name):
    c = C.case(name)
    h = R.rgb_to_hsv(C.before_hsv(c))[..., 0].astype(np.float64)
    d = c['p']['hue']
    assert ((h > 0) & (h < 0.032)).any() and ((h > 1 - 0.032) & (h < 1)).any()
    wraps = (h + d >= 1) if d > 0 else (h + d < 0)
    assert wraps.any() and not wraps.all()


@pytest.mark.parametrize('name', _tagged('clip'))
def test_clip_cases_hold_pixels_on_both_bounds(name):
    assert (C.oracle(name) == 0).any() and (C.oracle(name) == 255).any()


def test_colour_cases_reach_their_branches():
    for name in _tagged('v0'):
        pre = C.before_hsv(C.case(name))
        v, span = pre.max(-1), pre.max(-1) - pre.min(-1)
        assert (v == 0).any() and ((span == 0) & (v > 0)).any() and (span > 0).any(), name
    for name in _tagged('below0'):
        pre = C.before_hsv(C.case(name))
        assert (pre.max(-1) < 0).any() and (pre < 0).any() and (pre > 0).any(), name       # a negative v too
    for name in _tagged('above255'):
        assert (C.before_hsv(C.case(name)) > 255).any(), name
    for name in _tagged('satclip'):
        c = C.case(name)
        s = R.rgb_to_hsv(C.before_hsv(c))[..., 1]
        assert (s * np.float32(c['p']['saturation']) > 1).any() and (s * np.float32(c['p']['saturation']) < 1).any(), name
    for name in _tagged('sectors'):
        hsv = R.rgb_to_hsv(C.before_hsv(C.case(name)))
        assert set(np.unique((hsv[..., 0] * np.float32(6)).astype(int))) >= set(range(6)), name
        top = np.sort(C.case(name)['src'].reshape(-1, 3), -1)
        assert ((top[:, 2] == top[:, 1]) & (top[:, 1] > top[:, 0])).any()            # two equal maxima
        assert {tuple(p) for p in C.PALETTE[:6]} <= {tuple(p) for p in C.case(name)['src'].reshape(-1, 3)}
    for name in _tagged('mean'):
        c = C.case(name)
        mean = F.resize(c['src'], c['H'], c['W']).mean((0, 1))
        assert (mean.astype(np.float32).astype(np.float64) != mean).all(), name            # not an f32 number
    for name in _tagged('grey'):
        o = C.oracle(name)
        assert np.array_equal(o[..., 0], o[..., 1]) and np.array_equal(o[..., 1], o[..., 2]) and o.std() > 1, name
    for name in [n for n in C.NAMES if {'copy', 'int_down'} & C.IMAGES[n][4]]:
        np.testing.assert_array_equal(C.oracle(name), C.exact_expectation(C.case(name)), err_msg=name)
        np.testing.assert_array_equal(C.f64(name), C.exact_expectation(C.case(name)), err_msg=name)
    assert any(C.case(n)['p'].get('crop', (0, 0))[:2] != (0, 0) for n in _tagged('copy'))      # the shortcut at a non-zero crop_x / crop_y


# ---------------------------------------------------------------------------------------------------------------------
# labels: the host port (the specification the device is held to, bit for bit) against the float64 reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', C.LABELS)
def test_host_labels_vs_f64(name):
    from yolo_tf_amd.utils import data
    L = C.labels(name)
    errs = 0
    for b, (cls, box) in enumerate(L['objs']):
        ref = C.labels_f64(name)[b][0]
        errs |= ref[6]
        if ref[6]:
            with pytest.raises(IndexError):
                data.transform_labels(cls, box, L['classes'], L['cw'], L['ch'])
            continue
        C.assert_labels_match_f64(data.transform_labels(cls, box, L['classes'], L['cw'], L['ch']), name, b)
    assert errs == L['err']


def test_label_cases_reach_what_their_ids_say():
    ref = lambda name, b=0: C.labels_f64(name)[b][0]
    grids = {(C.labels(n)['cw'], C.labels(n)['ch'], C.labels(n)['classes']) for n in C.LABELS}
    assert {(1, 1, 1), (19, 19, 80), (7, 20, 1), (20, 7, 1)} <= grids
    mask, _, coords, _, _, _, _ = ref('centre_on_cell_boundary')
    assert mask[2 * 20 + 5] == 1 and coords[2 * 20 + 5, 0] == 0 and mask[5] == 1 and mask.sum() == 2       # exactly on the line: the right cell
    mask, _, coords, lo, hi, areas, _ = ref('zero_extent')
    assert mask.sum() == 3 and (areas == 0).all() and (coords[mask == 1, 2:] == 0).sum() == 4
    mask, _, _, _, _, _, err = ref('centre_x_1_wraps_a_row')
    assert err == 0 and mask[5 * 13] == 1 and mask[13] == 1 and mask.sum() == 2      # centre x == 1.0: column 0 of the NEXT row
    mask, _, _, _, _, _, err = ref('centre_1_1_out_of_range')
    assert err == 1 and mask.sum() == 0
    mask, prob, coords, _, _, _, _ = ref('three_in_one_cell')
    box = C.labels('three_in_one_cell')['objs'][0][1].astype(np.float64)
    assert mask.sum() == 1 and prob.sum() == 3 and coords[mask == 1, 2] == np.sqrt(box[2, 2] - box[2, 0])      # the last box's numbers
    counts = [len(c) for c, _ in C.labels('b33_ragged')['objs']]
    assert len(counts) == 33 and counts[0] == 0 and counts[-1] == 0 and max(counts) == 60
    assert ref('sticky_error_in_image_0', 0)[6] == 1 and not any(ref('sticky_error_in_image_0', b)[6] for b in (1, 2, 3))


# ---------------------------------------------------------------------------------------------------------------------
# image and boxes stay together
# ---------------------------------------------------------------------------------------------------------------------
TIE_SRC_W, TIE_SRC_H, TIE_W, TIE_H = 200, 160, 144, 112
TIE_BOXES = np.array([[120, 90, 175, 140], [95, 70, 150, 115], [130, 75, 170, 100]], np.float32)       # one colour channel each; all right of and below the centre


def _painted_box(img, channel):
    on = img[..., channel] >= 127.5
    ys, xs = np.flatnonzero(on.any(1)), np.flatnonzero(on.any(0))
    return np.array([xs[0], ys[0], xs[-1] + 1, ys[-1] + 1], np.float64)


def test_image_and_boxes_stay_together():
    """Boxes painted into the source, cropped / resized / flipped by the oracle's image path with augment.draw's parameters, must lie where
    augment.draw's box arithmetic puts them.  Per edge the two may differ by 1 + 4 * max(1, W / crop_w) output pixels (in y: H / crop_h):
    paint rounding, the integer truncation of the crop origin and of its extent, one source pixel of interpolation ramp -- four terms of
    at most one source pixel, each W / crop_w output pixels (at least one) -- and one output pixel of sampling.  A draw is used only if a
    mirrored box, and with a crop a box without the crop's shift, would miss by more than three times that bound, which the test asserts
    of its inputs; the selection looks at the draw alone, never at the image."""
    from yolo_tf_amd.utils import augment as A
    ini = configparser.ConfigParser()
    ini.read(os.path.join(ROOT, 'config.ini'))
    cfg = A.AugmentConfig(ini)
    src = np.zeros((TIE_SRC_H, TIE_SRC_W, 3), np.uint8)
    for ch, (x0, y0, x1, y1) in enumerate(TIE_BOXES.astype(int)):
        src[y0:y1, x0:x1, ch] = 255
    seen = {}
    for seed in range(200):
        p, norm = A.draw(cfg, np.random.RandomState(seed), (TIE_SRC_W, TIE_SRC_H), TIE_BOXES, TIE_W, TIE_H)
        cropped, flipped = p['crop'] != (0, 0, TIE_SRC_W, TIE_SRC_H), bool(p['flags'] & A.FLIP)
        if seen.get((cropped, flipped), 0) >= 3:
            continue
        cx, cy, cw, ch_ = p['crop']
        sx, sy = TIE_W / cw, TIE_H / ch_
        bound = np.array([1 + 4 * max(1, sx), 1 + 4 * max(1, sy)] * 2)
        box = norm.astype(np.float64) * [TIE_W, TIE_H, TIE_W, TIE_H]
        mirror_miss = np.abs(TIE_W - box[:, 0] - box[:, 2])                           # how far the mirrored box's edges are from the box's
        shift_miss = max(cx * sx / bound[0], cy * sy / bound[1])
        if not (mirror_miss > 3 * bound[0]).all() or (cropped and shift_miss <= 3) or (box[:, 2] - box[:, 0] < 16).any():
            continue
        seen[(cropped, flipped)] = seen.get((cropped, flipped), 0) + 1
        # the properties of the inputs, asserted
        assert (box[:, 2] - box[:, 0] >= 16).all() and (box[:, 3] - box[:, 1] >= 16).all()
        assert (mirror_miss > 3 * bound[0]).all() and (not cropped or shift_miss > 3)
        img = R.augment_image(src, dict(crop=p['crop'], flip=flipped), TIE_W, TIE_H)
        for k in range(len(TIE_BOXES)):
            got = _painted_box(img, k)
            assert (np.abs(got - box[k]) <= bound).all(), 'seed %d box %d: painted %s, returned %s, bound %s' % (seed, k, got, box[k], bound)
            mirrored = np.array([TIE_W - box[k, 2], box[k, 1], TIE_W - box[k, 0], box[k, 3]])
            assert (np.abs(got - mirrored) > bound).any()                             # and the test can tell: the mirrored box is not accepted
    assert all(seen.get(k, 0) >= 2 for k in ((False, False), (False, True), (True, False), (True, True))), seen
    assert sum(seen.values()) >= 8
