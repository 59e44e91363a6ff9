"""The IoU-family box losses without a GPU: the specification's hand-derived gradient against torch float64 autograd of its own forward, the
conditions under which a correct kernel and the float64 specification must agree on every case of tests/box_loss_cases.py, and the proof
that the bounds of tests/test_box_loss_gpu.py catch wrong losses (the mutations at the end)."""
import numpy as np
import pytest
import torch

import box_loss_cases as BC
import box_loss_ref as S
import head_cases as H
from oracle import yolo2_ref as R

CASE_MODES = [(n, m) for n in BC.CASES for m in BC.modes(n)]
SMALL = [(n, m) for n, m in CASE_MODES if n != 'b8_19x19']       # (the largest case; its mechanism is the workgroup count, which no mutation concerns)


# ---------------------------------------------------------------------------------------------------------------------
# the specification itself
# ---------------------------------------------------------------------------------------------------------------------

def test_mse_is_the_oracle():
    c = BC.case('sq13_ld136')
    obj, _, dl = S.loss(H.inputs64(c['net'], 'f32'), c['labels'], c['anchors'], H.HP, c['C'], 'mse')
    ref = H.v2_reference('sq13_ld136', 'f32')
    assert obj == ref['obj'] and np.array_equal(dl, ref['dlogits'])


@pytest.mark.parametrize('name,mode,method', [(n, 'f32' if 'f32' in BC.modes(n) else 'bf16', k) for n in BC.CASES for k in BC.METHODS])
def test_analytic_gradient_vs_autograd(name, mode, method):
    """d(hparam.coords * coords objective)/d logits by torch float64 autograd through sigmoid, exp and the specification's own forward
    (box_loss_ref.score with xp = torch; mask_best and alpha are constants), against loss_backward's channels 1..4."""
    c, ref = BC.case(name), BC.reference(name, mode, method)
    B, cells, A = c['B'], c['ch'] * c['cw'], c['A']
    mb = ref['aux']['mask_best']
    b, cell, a = np.nonzero(mb)
    z = torch.tensor(H.inputs64(c['net'], mode).reshape(B, cells, A, -1)[b, cell, a, 1:5], dtype=torch.float64, requires_grad=True)
    anchors = torch.tensor(c['anchors'].astype(np.float64)[a])
    lab = [torch.tensor(np.asarray(l, np.float64)[b, cell, 0]) for l in c['labels']]
    tmin, tmax, tareas = lab[3], lab[4], lab[5]
    sx, sy = torch.sigmoid(z[:, 0]), torch.sigmoid(z[:, 1])
    w, h = torch.exp(z[:, 2]) * anchors[:, 0], torch.exp(z[:, 3]) * anchors[:, 1]
    q = S.score(torch, method, sx, sy, w, h, tmin[:, 0], tmin[:, 1], tmax[:, 0], tmax[:, 1], tareas)
    cnt = float(B * cells * A)
    coords = (1 - q).sum() / cnt
    assert abs(float(coords.detach()) - float(ref['obj']['coords'])) <= 1e-12 * abs(float(ref['obj']['coords'])) + 1e-300
    (H.HP['coords'] * coords).backward()
    got = BC.box_channels(c, ref['dlogits']).reshape(B, cells, A, 4)
    want = np.zeros_like(got)
    want[b, cell, a] = z.grad.numpy()
    assert np.all(np.isfinite(got))
    err = np.abs(got - want).max()
    print('%s %s %s: |analytic - autograd| max %.3e of max %.3e' % (name, mode, method, err, np.abs(want).max()))
    assert err <= 1e-11 * np.abs(want).max() + 1e-300
    assert np.all(got[mb == 0] == 0)


def test_alpha_is_a_constant_and_v_has_its_true_derivative():
    """Differentiating through alpha gives another gradient (so the check above does distinguish the two), and the CIoU term is live."""
    ref, mut = BC.reference('inside', 'f32', 'ciou'), BC.reference('inside', 'f32', 'ciou', np.float64, 'alpha_grad')
    c = BC.case('inside')
    assert H.f32_ratio(BC.box_channels(c, mut['dlogits']), BC.box_channels(c, ref['dlogits'])) > 1.0
    diou = BC.reference('inside', 'f32', 'diou')
    assert H.f32_ratio(BC.box_channels(c, diou['dlogits']), BC.box_channels(c, ref['dlogits'])) > 1.0


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_a_box_that_underflowed_to_nothing_leaves_the_gradient_finite(dtype):
    """exp(z3) = exp(z4) = 0 on responsible lanes (logits of -120 underflow in float32; -800 in float64): w^2 + h^2 is floored in the derivative
    of v like the other denominators, so every mode's dlogits stay finite and the size channels get exactly zero."""
    c = BC.case('a1')
    for method in BC.METHODS:
        obj, aux, dl = S.loss(BC.zero_box_net(c, -800.0 if dtype == np.float64 else -120.0).astype(dtype), c['labels'], c['anchors'], H.HP, c['C'], method)
        g = BC.box_channels(c, dl).reshape(c['B'], -1, c['A'], 4)
        resp = aux['mask_best'] != 0
        assert resp.sum() >= 8 and np.all(aux['box_args'][2][resp] == 0) and np.all(aux['box_args'][3][resp] == 0)
        assert np.all(np.isfinite(dl)) and np.isfinite(obj['coords']) and np.all(g[resp][:, 2:] == 0), method


# ---------------------------------------------------------------------------------------------------------------------
# conditions on the cases
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,mode', CASE_MODES)
def test_everything_but_the_box_term_is_the_oracle(name, mode):
    c = BC.case(name)
    base = BC.reference(name, mode, 'mse')
    for method in BC.METHODS:
        ref = BC.reference(name, mode, method)
        assert np.array_equal(ref['aux']['mask_best'], base['aux']['mask_best'])
        for k in ('iou_best', 'iou_normal', 'prob'):
            assert ref['obj'][k] == base['obj'][k]
        assert np.array_equal(BC.other_channels(c, ref['dlogits']), BC.other_channels(c, base['dlogits']))
        assert np.all(np.isfinite(ref['dlogits'])) and np.isfinite(ref['obj']['coords']) and ref['obj']['coords'] > 0
        assert np.array_equal(ref['aux']['mask_best'].sum(2).astype(np.int64), c['resp'])


@pytest.mark.parametrize('name,mode', CASE_MODES)
def test_responsible_lanes_are_away_from_every_kink(name, mode):
    d = BC.kink_distance(name, mode)
    print('%s %s: smallest distance of a responsible lane from a kink %.3e' % (name, mode, d))
    assert d >= BC.KINK
    assert BC.smallest_r2(name, mode) >= 1e10 * S.R2_FLOOR          # the underflow guard of dv is ten orders of magnitude away
    # an empty intersection is intended in `disjoint` (and is `tie_all`'s construction), in both axes and far from the boundary; nowhere else is a
    # responsible lane's intersection empty in both axes by construction
    aux = BC.reference(name, mode, 'ciou')['aux']
    if name in ('disjoint', 'tie_all'):
        assert np.all(aux['iou'][aux['mask_best'] != 0] == 0)


@pytest.mark.parametrize('name,mode,method', BC.ALL)
def test_float32_specification_stays_within_a_quarter_of_the_bounds(name, mode, method):
    """Room for a kernel's own operation order: the float32 specification uses at most 0.25 of each bound against its float64 self, and makes
    the same choice of responsible anchors.  (bf16: the arithmetic before the store is held to 0.25 of the f32 bound; a round-to-nearest store
    may by itself use nearly all of bf16_ratio's 2^-8 |ref| next to a power of two, so the stored value is held to that bound, 1.0.)"""
    c = BC.case(name)
    ref, f32 = BC.reference(name, mode, method), BC.reference(name, mode, method, np.float32)
    assert np.array_equal(f32['aux']['mask_best'], ref['aux']['mask_best'])
    assert np.all(np.isfinite(f32['dlogits'])) and np.isfinite(f32['obj']['coords'])
    r_obj = H.objective_ratio(f32['obj']['coords'], ref['obj']['coords'])
    g, g32 = BC.box_channels(c, ref['dlogits']), BC.box_channels(c, f32['dlogits'])
    r_grad = H.f32_ratio(g32, g) if np.abs(g).max() > 0 else float(np.abs(g32).max() > 0)
    print('%s %s %s: float32 specification uses %.3f of the objective bound, %.3f of the gradient bound' % (name, mode, method, r_obj, r_grad))
    assert r_obj <= BC.F32_SELF
    if name in BC.GRADIENT_CONDITION_EXEMPT:
        return
    assert r_grad <= BC.F32_SELF
    if mode == 'bf16' and np.abs(g).max() > 0:
        assert H.bf16_ratio(H.stored(g32, 'bf16'), g) <= 1.0


def test_placed_cases_are_what_they_say():
    for mode in H.MODES:
        # disjoint: five responsible anchors with IoU exactly 0; the iou mode's gradient is exactly zero, the others' is not
        c = BC.case('disjoint')
        ref = BC.reference('disjoint', mode, 'iou')
        obj_cells = c['labels'][0][..., 0] != 0
        assert np.all(ref['aux']['mask_best'].sum(2)[obj_cells] == 5) and np.all(ref['aux']['iou'][obj_cells] == 0)
        assert np.all(BC.box_channels(c, ref['dlogits']) == 0)
        for method in ('giou', 'diou', 'ciou'):
            g = BC.box_channels(c, BC.reference('disjoint', mode, method)['dlogits']).reshape(c['B'], -1, c['A'], 4)
            assert np.all(np.abs(g[ref['aux']['mask_best'] != 0]).max(-1) > 0)
        # inside: GIoU equals IoU, IoU has no centre gradient, DIoU has one
        c = BC.case('inside')
        iou, giou, diou = (BC.reference('inside', mode, k) for k in ('iou', 'giou', 'diou'))
        assert abs(giou['obj']['coords'] - iou['obj']['coords']) <= 1e-6 * iou['obj']['coords']       # (E is the target's area up to the f32 rounding of the `areas` label)
        mb = iou['aux']['mask_best'] != 0
        assert np.all(BC.box_channels(c, iou['dlogits']).reshape(c['B'], -1, c['A'], 4)[mb][:, :2] == 0)
        assert np.all(np.abs(BC.box_channels(c, diou['dlogits']).reshape(c['B'], -1, c['A'], 4)[mb][:, :2]) > 0)
        # inside and encloses: the winner's aspect ratio differs from the target's by at least 15 %, so CIoU is not DIoU
        for name in ('inside', 'encloses'):
            aux = BC.reference(name, mode, 'ciou')['aux']
            sx, sy, w, h, X1, Y1, X2, Y2, At = [np.broadcast_to(a, aux['mask_best'].shape)[aux['mask_best'] != 0] for a in aux['box_args']]
            ratio = (w / h) / ((X2 - X1) / (Y2 - Y1))
            assert len(ratio) == 10 and np.all(np.maximum(ratio, 1 / ratio) >= 1.15), ratio
            cc = BC.case(name)
            assert H.f32_ratio(BC.box_channels(cc, BC.reference(name, mode, 'diou')['dlogits']), BC.box_channels(cc, BC.reference(name, mode, 'ciou')['dlogits'])) > 1.0
        # encloses: every prediction contains its target
        aux = BC.reference('encloses', mode, 'iou')['aux']
        sx, sy, w, h, X1, Y1, X2, Y2, At = [np.broadcast_to(a, aux['mask_best'].shape)[aux['mask_best'] != 0] for a in aux['box_args']]
        assert np.all(sx - w / 2 < X1) and np.all(sx + w / 2 > X2) and np.all(sy - h / 2 < Y1) and np.all(sy + h / 2 > Y2)


# ---------------------------------------------------------------------------------------------------------------------
# Teeth.  A kernel's output is modelled as the exact (float64) result of a computation, stored in the kernel's dtype.  The specification
# stays inside the GPU test's bounds on every case; each wrong loss leaves them on at least one.
# ---------------------------------------------------------------------------------------------------------------------

def _ratios(name, mode, method, got):
    """(objective ratio, gradient ratio) of a modelled kernel output `got` (a reference dict) against the specification."""
    c, ref = BC.case(name), BC.reference(name, mode, method)
    g = BC.box_channels(c, ref['dlogits'])
    r_grad = H.grad_ratio(H.stored(BC.box_channels(c, got['dlogits']), mode), g, mode) if np.abs(g).max() > 0 else 0.0
    return H.objective_ratio(got['obj']['coords'], ref['obj']['coords']), r_grad


@pytest.mark.parametrize('name,mode,method', BC.ALL)
def test_a_correct_store_of_the_exact_result_fits_the_bounds(name, mode, method):
    r_obj, r_grad = _ratios(name, mode, method, BC.reference(name, mode, method))
    assert r_obj == 0 and r_grad <= 1.0


def _caught(mutation, method):
    out = {}
    for name, mode in SMALL:
        r_obj, r_grad = _ratios(name, mode, method, BC.reference(name, mode, method, np.float64, mutation))
        if max(r_obj, r_grad) > 1.0:
            out[(name, mode)] = max(r_obj, r_grad)
    return out


@pytest.mark.parametrize('mutation,method', [('alpha_grad', 'ciou'), ('no_w_factor', 'iou'), ('no_w_factor', 'giou'), ('no_w_factor', 'diou'),
                                             ('no_w_factor', 'ciou'), ('c_not_c2', 'diou'), ('c_not_c2', 'ciou'), ('enclose_intersection', 'giou'),
                                             ('enclose_intersection', 'diou'), ('enclose_intersection', 'ciou'), ('mask_not_best', 'iou'),
                                             ('mask_not_best', 'giou'), ('mask_not_best', 'diou'), ('mask_not_best', 'ciou')])
def test_every_mutation_leaves_the_bounds_somewhere(mutation, method):
    caught = _caught(mutation, method)
    print('%s %s: %d of %d; %s' % (mutation, method, len(caught), len(SMALL), ', '.join('%s %s %.3g' % (n, m, r) for (n, m), r in sorted(caught.items())[:6])))
    assert caught
    if mutation == 'mask_not_best':       # (one anchor, or all of them responsible: mask == mask_best)
        assert not {'a1', 'tie_all', 'disjoint'} & {n for n, _ in caught}


def test_mutation_bf16_truncation():
    for method in BC.METHODS:
        caught = []
        for name, mode in CASE_MODES:
            c = BC.case(name)
            g = BC.box_channels(c, BC.reference(name, mode, method)['dlogits'])
            if mode == 'bf16' and np.abs(g).max() > 0:
                assert H.bf16_ratio(H.stored(g, mode), g) <= 1.0
                if H.bf16_ratio(H.stored(g, mode, H.bf16_truncate), g) > 1.0:
                    caught.append(name)
        print('%s: truncation leaves the bound on %d cases' % (method, len(caught)))
        assert caught


@pytest.mark.parametrize('method,other', [(a, b) for a in BC.METHODS for b in BC.METHODS if a != b])
def test_each_method_in_place_of_each_other_leaves_the_bounds(method, other):
    caught = [(n, m) for n, m in SMALL if max(_ratios(n, m, method, BC.reference(n, m, other))) > 1.0]
    print('%s computed where %s was asked for: caught on %d of %d' % (other, method, len(caught), len(SMALL)))
    assert caught
