"""The head-kernel cases of tests/head_cases.py, checked without a GPU: every input is one on which a correct kernel and the float64 oracle
must agree (no near-tie of the two best IoUs in any object cell, the intended number of responsible anchors, finite references), and
every bound of tests/test_head_gpu.py is one a subtly wrong kernel leaves (the mutations at the end)."""
import numpy as np
import pytest

import head_cases as H
from oracle import yolo2_ref as R

V2 = [(n, m) for n in H.V2_SPECS for m in H.V2_SPECS[n][8]]
V1 = [(n, m) for n in H.V1_SPECS for m in H.MODES]


def _finite(tree):
    if isinstance(tree, dict):
        return all(_finite(v) for v in tree.values())
    return bool(np.all(np.isfinite(np.asarray(tree, np.float64))))


def _check_margins(case, ref):
    mask = case['labels'][0]
    objects = int(mask.sum())
    assert objects >= 8, objects
    per_cell = H.margins(ref['iou'], mask)
    assert len(per_cell) == objects
    gaps = [g for _, g in per_cell]
    print('%s: %d object cells, smallest relative gap below the best IoU %.3e' % (case['name'], objects, min(gaps)))
    assert min(gaps) > H.MARGIN, min(gaps)                      # every object cell, none excluded
    # responsible anchors per cell: what the construction intends, what the oracle's mask_best says
    assert np.array_equal(np.array([n for n, _ in per_cell]), case['resp'][mask[..., 0] != 0])
    assert np.array_equal(ref['aux']['mask_best'].sum(2).astype(np.int64), case['resp'])


@pytest.mark.parametrize('name,mode', V2)
def test_v2_case_conditions(name, mode):
    c, ref = H.v2_case(name), H.v2_reference(name, mode)
    assert c['ld'] >= c['D'] and c['net'].shape == (c['B'], c['ch'], c['cw'], c['D']) and c['net'].dtype == np.float32
    assert all(l.dtype == np.float32 and l.shape[:2] == (c['B'], c['ch'] * c['cw']) for l in c['labels'])
    assert _finite(ref['m']) and _finite(ref['obj']) and _finite(ref['dlogits'])
    assert all(float(v) > 0 for v in ref['obj'].values())       # a purely relative bound on each objective is meaningful
    _check_margins(c, ref)
    # the f32 oracle on the same values makes the same choice and computes the same objectives
    f32 = H.v2_reference(name, mode, np.float32)
    assert np.array_equal(f32['aux']['mask_best'], ref['aux']['mask_best'])
    for k in R.OBJECTIVE_KEYS:
        assert H.objective_ratio(f32['obj'][k], ref['obj'][k]) <= 1.0, k
    # nothing overflows in f32 on the big logits either (overflow is check_numerics territory: test_head_decode_f32 and the flag tests)
    assert _finite(f32['m']) and _finite(f32['dlogits'])


def test_v2_tie_counts():
    """6a: five responsible anchors in every object cell.  6b: two where the identical pair is the best, one where it is not, both kinds present."""
    for mode in H.MODES:
        a, b = H.v2_case('tie_all'), H.v2_case('tie_pair')
        mb = H.v2_reference('tie_all', mode)['aux']['mask_best']
        assert np.all(mb.sum(2)[a['labels'][0][..., 0] != 0] == 5)
        assert np.all(H.v2_reference('tie_all', mode)['iou'][a['labels'][0][..., 0] != 0] == 0)
        mb = H.v2_reference('tie_pair', mode)['aux']['mask_best']
        n = mb.sum(2)[b['labels'][0][..., 0] != 0]
        assert sorted(set(n.tolist())) == [1, 2] and (n == 2).sum() >= 4 and (n == 1).sum() >= 4
        two = mb[mb.sum(2) == 2]
        assert np.all(two[:, 1] == 1) and np.all(two[:, 3] == 1)                 # the pair itself
        assert np.all(mb[mb.sum(2) == 1][:, [1, 3]] == 0)                        # and not the pair elsewhere


def test_v2_shapes_reach_every_lane_group():
    lpc = lambda a: 1 << (a - 1).bit_length()
    assert {lpc(H.V2_SPECS[n][3]) for n in H.V2_SPECS} == {1, 2, 4, 8, 16, 64}
    c = H.v2_case('b8_19x19')
    threads = c['B'] * c['ch'] * c['cw'] * 8
    assert (threads + 255) // 256 == 91 and threads % 256 != 0                   # the finalisation's 64-lane loop wraps; the last workgroup is partly idle
    assert H.v2_case('a8')['ld'] == H.v2_case('a8')['D'] == 72 and H.v2_case('a8_ld80')['ld'] == 80
    assert np.array_equal(H.v2_case('a8')['net'], H.v2_case('a8_ld80')['net'])
    assert H.v2_case('sq13_ld136')['ld'] == H.pad8(125) + 8
    big = H.v2_case('rect19x11')['net'].reshape(-1, 25)
    assert big[:, 3:5].min() == -6 and big[:, 3:5].max() == 4 and np.abs(big[:, 5:]).max() > 24 and np.abs(big[:, :3]).max() > 15


@pytest.mark.parametrize('name,mode', V1)
def test_v1_case_conditions(name, mode):
    c, ref = H.v1_case(name), H.v1_reference(name, mode)
    assert c['net'].shape == (c['B'], c['width']) and c['ld'] >= c['width']
    assert _finite(ref['m']) and _finite(ref['obj']) and _finite(ref['dnet'])
    assert all(float(v) > 0 for v in ref['obj'].values())
    _check_margins(c, ref)
    f32 = H.v1_reference(name, mode, np.float32)
    assert np.array_equal(f32['aux']['mask_best'], ref['aux']['mask_best'])
    for k in R.OBJECTIVE_KEYS:
        assert H.objective_ratio(f32['obj'][k], ref['obj'][k]) <= 1.0, k
    # the |x| gradient at exactly 0 is exercised by a responsible box, and a tie by two identical boxes
    base, mb = ref['m']['wh01_sqrt_base'], ref['aux']['mask_best']
    assert np.all(base[c['zero_cell']][:, 0] == 0) and np.all(mb[c['zero_cell']] == 1)
    if c['boxes'] > 1:
        assert np.array_equal(base[c['tie_cell']][0], base[c['tie_cell']][1]) and ref['iou'][c['tie_cell']][0] > 0.9
        assert np.all(mb[c['tie_cell']][:2] == 1) and np.all(mb[c['tie_cell']][2:] == 0)


def test_bf16_round_is_round_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -1.0 - 2.0 ** -7 + 2.0 ** -20], np.float32)
    r = R.bf16_round(x)
    assert r[0] == 1 and r[1] == 1 and r[2] == 1 + 2.0 ** -6 and r[3] == 1 + 2.0 ** -7 and r[4] == -1 - 2.0 ** -7
    assert np.all(np.abs(r.astype(np.float64) - x) <= H.BF16_HALF_ULP * np.abs(x))
    t = H.bf16_truncate(x)
    assert t[3] == 1 and t[4] == -1


# ---------------------------------------------------------------------------------------------------------------------
# Teeth.  A kernel's output is modelled as the exact (float64) result of a computation, stored in the kernel's dtype.  The correct
# computation stays inside the GPU test's bounds on every case; each wrong one leaves them on the cases built to show it.
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,mode', V2)
def test_restated_loss_is_the_oracle_and_fits_the_bounds(name, mode):
    ref = H.v2_reference(name, mode)
    obj, dl = H.v2_restated(name, mode)
    for k in R.OBJECTIVE_KEYS:
        assert abs(obj[k] - ref['obj'][k]) <= 1e-12 * abs(ref['obj'][k]), k
    assert np.abs(dl - ref['dlogits']).max() <= 1e-12 * np.abs(ref['dlogits']).max()
    ratio = H.grad_ratio(H.stored(dl, mode), ref['dlogits'], mode)
    print('%s %s: a correctly rounded store of the exact gradient uses %.3f of the bound' % (name, mode, ratio))
    assert ratio <= 1.0


def _caught(mutation):
    """{(case, mode): worst dlogits ratio} of the cases on which the mutated computation leaves the gradient bound."""
    out = {}
    for name, mode in V2:
        if name == 'b8_19x19':
            continue        # (the largest case; its mechanism is the workgroup count, which no mutation here concerns)
        _, dl = H.v2_restated(name, mode, mutation)
        ratio = H.grad_ratio(H.stored(dl, mode), H.v2_reference(name, mode)['dlogits'], mode)
        if ratio > 1.0:
            out[(name, mode)] = ratio
    return out


def _names(caught):
    return {n for n, _ in caught}


def test_mutation_cell_width_and_height_swapped():
    caught = _caught('swap_cell_wh')
    assert {('rect9x14', 'f32'), ('rect9x14', 'bf16'), ('rect19x11', 'f32'), ('rect19x11', 'bf16')} <= set(caught)
    assert 'sq13_ld136' not in _names(caught)       # invisible on a square grid: the only geometry the gradient was checked on before


def test_mutation_bf16_truncation():
    caught = []
    for name, mode in V2:
        if mode == 'bf16':
            ref = H.v2_reference(name, mode)['dlogits']
            assert H.bf16_ratio(H.stored(ref, mode), ref) <= 1.0
            if H.bf16_ratio(H.stored(ref, mode, H.bf16_truncate), ref) > 1.0:
                caught.append(name)
    assert set(caught) == {n for n, m in V2 if m == 'bf16'}       # thousands of elements each: some lose almost a whole ulp


def test_mutation_class_term_masked_by_mask():
    caught = _caught('class_mask')
    assert _names(caught) >= set(H.V2_SPECS) - {'a1', 'b8_19x19', 'tie_all'}      # (one anchor, or all of them responsible: mask == mask_best)
    assert not {'a1', 'tie_all'} & _names(caught)


def test_mutation_first_maximum_instead_of_all_equal():
    caught = _caught('first_max')
    assert _names(caught) == {'tie_all', 'tie_pair'} and len(caught) == 4


def test_mutation_iou_weights_swapped():
    assert _names(_caught('swap_iou_weights')) == set(H.V2_SPECS) - {'b8_19x19'}


def test_mutation_anchors_indexed_modulo_five():
    caught = _caught('anchor_mod5')
    assert _names(caught) == {'a8', 'a8_ld80', 'a9', 'a33'} and len(caught) == 8


@pytest.mark.parametrize('mutation', H.MUTATIONS)
def test_every_mutation_leaves_the_gradient_bound_somewhere(mutation):
    caught = _caught(mutation)
    print('%s: %s' % (mutation, ', '.join('%s %s %.3g' % (n, m, r) for (n, m), r in sorted(caught.items()))))
    assert caught
