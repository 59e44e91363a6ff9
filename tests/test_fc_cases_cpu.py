"""The fully connected cases of tests/fc_cases.py, checked without a GPU: every reference is finite and of unit scale, both branches of the
leaky-ReLU are exercised, the f32 oracle agrees with the float64 one inside the f32 bound, the launch rule (queried on the host at 256 CUs) sends
every case down the branch it is named for, and every bound of tests/test_fc_gpu.py is one a subtly wrong kernel leaves (the mutations)."""
import numpy as np
import pytest
import torch

import fc_cases as F

TDTYPE = {'f32': torch.float32, 'bf16': torch.bfloat16}
FWD = [(n, m, e) for n in F.FWD_SPECS for m in F.MODES for e in F.EPILOGUES]
SLICED = [(n, m) for n in F.FWD_SPECS for m in F.MODES if F.sliced(n, m)]
WGRAD = [(n, m) for n in F.WGRAD_SPECS for m in F.MODES]
BIAS_GRAD = [(n, m) for n in F.BIAS_GRAD_SPECS for m in F.MODES]


@pytest.fixture(scope='module')
def ops():
    from yolo_tf_amd import ops as _ops
    _ops._lib.load()
    return _ops


def route(ops, name, mode, epilogue='plain', ws=True, deterministic=False):
    c = F.fwd_case(name)
    ops.set_deterministic(1 if deterministic else 0)
    try:
        return ops.conv_route(c['B'], 1, 1, F.FWD_SPECS[name][1], F.FWD_SPECS[name][1], c['Nf'], c['ldo'], 1, TDTYPE[mode],
                              'plain' if epilogue == 'plain' else 'bias_act', 4 * F.WS_FLOATS if ws else 0, cus=F.CUS)
    finally:
        ops.set_deterministic(0)


def slices_of(ops, name, mode):
    r = route(ops, name, mode)
    assert F.branch_of(r['plan']) == 'sliced' and r['plan']['grid_y'] > 1, r
    return r['plan']['grid_y']


def unit_scale(ref, what):
    assert np.all(np.isfinite(ref)), what
    top = float(np.abs(ref).max())
    assert 1.0 <= top <= 10.0, (what, top)


# ---------------------------------------------------------------------------------------------------------------------
# the cases themselves
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,mode,epilogue', FWD)
def test_forward_case_conditions(name, mode, epilogue):
    c, ref = F.fwd_case(name), F.fwd_reference(name, mode, epilogue)
    assert c['x'].shape == (c['B'], c['C']) and c['w'].shape == (c['C'], c['Nf']) and c['ldo'] % 8 == 0 and 0 <= c['ldo'] - c['Nf'] < 8
    assert F.FWD_SPECS[name][1] % 8 == 0 and 0 <= F.FWD_SPECS[name][1] - c['C'] < 8
    unit_scale(ref['y'], (name, mode, epilogue))
    if epilogue == 'bias_leaky':
        neg = float((ref['pre'] < 0).mean())
        print('%s %s: %.1f %% of %d pre-activations negative' % (name, mode, 100 * neg, ref['pre'].size))
        assert 0.3 <= neg <= 0.7, (name, mode, neg)
        assert np.array_equal(ref['y'], np.where(ref['pre'] < 0, F.ALPHA * ref['pre'], ref['pre']))
    f32 = F.fwd_reference(name, mode, epilogue, np.float32)['y']
    assert f32.dtype == np.float32
    ratio = F.f32_ratio(f32, ref['y'])
    print('%s %s %s: the f32 oracle uses %.3f of the f32 bound' % (name, mode, epilogue, ratio))
    assert ratio <= 1.0
    # a correctly rounded store of the exact result fits the bound of its dtype
    assert F.out_ratio(F.stored(ref['y'], mode), ref['y'], mode) <= 1.0


@pytest.mark.parametrize('name,mode', WGRAD)
def test_filter_gradient_case_conditions(name, mode):
    c, ref = F.wgrad_case(name), F.wgrad_reference(name, mode)
    assert ref.shape == (c['Cin'], c['Cout'])
    unit_scale(ref, (name, mode))
    f32 = F.wgrad_of(c, mode, np.float32)
    assert f32.dtype == np.float32 and F.f32_ratio(f32, ref) <= 1.0
    assert F.wgrad_ratio(ref.astype(np.float32), ref, mode) <= 1.0
    if c['B'] == 1 and mode == 'bf16':
        # one product of two bf16 values per element: exact in f32, so the GPU test may demand equality
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)


@pytest.mark.parametrize('name,mode', BIAS_GRAD)
def test_bias_gradient_case_conditions(name, mode):
    c, ref = F.bias_grad_case(name), F.bias_grad_reference(name, mode)
    assert ref.shape == (c['C'],) and c['ld'] >= c['C'] and c['ld'] % 8 == 0
    unit_scale(ref, (name, mode))
    assert F.f32_ratio(F.bias_grad_reference(name, mode, np.float32), ref) <= 1.0


def test_bias_gradient_cases_reach_both_kernels():
    """yolo2_bias_grad: ld / vec > 256 takes the thread-per-column kernel, else a workgroup per 16-byte channel group (csrc/bn_stats.hip)."""
    forms = {(n, m): F.BIAS_GRAD_SPECS[n][2] // (8 if m == 'bf16' else 4) > 256 for n, m in BIAS_GRAD}
    assert forms == {('db_b1', 'f32'): False, ('db_b1', 'bf16'): False, ('db_b3', 'f32'): True, ('db_b3', 'bf16'): True,
                     ('db_b8', 'f32'): True, ('db_b8', 'bf16'): False}


# ---------------------------------------------------------------------------------------------------------------------
# the launch rule's answer for every case (the library, no device)
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,mode,epilogue', FWD)
def test_route_pin_forward(ops, name, mode, epilogue):
    for ws, det in ((True, False), (False, False), (True, True)):
        r = route(ops, name, mode, epilogue, ws, det)
        want = F.expected_branch(name, mode, ws, det)
        assert r['family'] == 'igemm' and r['stats'] == 'none' and r['pending'] == 0, r
        assert F.branch_of(r['plan']) == want, (name, mode, epilogue, ws, det, r['plan'])
        assert all(r['plan'][k] == v for k, v in F.BRANCHES[want].items())
        assert (r['plan']['grid_y'] > 1) == (want == 'sliced') and (want == 'sliced' or r['plan']['grid_y'] == 1)
        tiles = -(-F.FWD_SPECS[name][3] // r['plan']['BN'])
        assert r['plan']['grid_x'] == tiles, r              # B <= 8: one row tile
    if F.sliced(name, mode):
        # >= 128 K steps, and every slice holds at least one
        assert F.FWD_SPECS[name][1] // F.k_step(mode) >= 128
        F.slice_bounds(F.fwd_case(name)['C'], mode, slices_of(ops, name, mode))


def test_route_pin_covers_every_branch_in_both_dtypes():
    for mode in F.MODES:
        assert {F.expected_branch(n, mode) for n in F.FWD_SPECS} == set(F.BRANCHES)
    assert F.sliced('k2048_b5', 'f32') and not F.sliced('k2048_b5', 'bf16')      # the threshold of 128 K steps, from both sides
    assert len(SLICED) == 9


@pytest.mark.parametrize('name,mode', WGRAD)
def test_route_pin_filter_gradient(ops, name, mode):
    B, Cin, Cout, _ = F.WGRAD_SPECS[name]
    plan = ops.wgrad_ws_plan(B, 1, 1, Cin, F.pad8(Cin), Cout, F.pad8(Cout), 1, TDTYPE[mode], F.CUS)
    assert plan['family'] == 3 and plan['slots'] == 1, plan
    small = Cin <= 64 or Cout <= 64 or -(-Cin // 128) * -(-Cout // 128) < 33      # conv_wgrad.hip wgrad_small_tile
    tile = 64 if small else 128
    assert plan['blocks'] == -(-Cin // tile) * -(-Cout // tile), plan
    assert small == (name == 'w_b1_c520')
    # wgrad_per_tap: the bf16 launch takes the 64-pixel reduction tile while 2 * blocks <= 3 * CUs
    assert (2 * plan['blocks'] <= 3 * F.CUS) == (name != 'w_b2_big')
    assert 45 <= plan['blocks'] <= 512


# ---------------------------------------------------------------------------------------------------------------------
# Teeth.  A kernel's output is modelled as the exact (float64) result of a computation, stored in the kernel's dtype.  The correct
# computation stays inside the GPU test's bounds on every case; each wrong one leaves them on every case it applies to.
# ---------------------------------------------------------------------------------------------------------------------

def stored_ratio(wrong64, name, mode, epilogue):
    return F.out_ratio(F.stored(wrong64, mode), F.fwd_reference(name, mode, epilogue)['y'], mode)


@pytest.mark.parametrize('name,mode', SLICED)
def test_sum_of_slices_is_the_reference(ops, name, mode):
    n = slices_of(ops, name, mode)
    for e in F.EPILOGUES:
        ref = F.fwd_reference(name, mode, e)['y']
        got = F.fwd_by_slices(name, mode, e, n)
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
        assert stored_ratio(got, name, mode, e) <= 1.0


@pytest.mark.parametrize('name,mode', SLICED)
def test_mutation_one_slice_dropped(ops, name, mode):
    n = slices_of(ops, name, mode)
    for e in F.EPILOGUES:
        for drop in (0, n // 2, n - 1):
            assert stored_ratio(F.fwd_by_slices(name, mode, e, n, drop=drop), name, mode, e) > 1.0, (e, drop)


@pytest.mark.parametrize('name,mode', SLICED)
def test_mutation_bias_added_once_per_slice(ops, name, mode):
    n = slices_of(ops, name, mode)
    for e in ('bias', 'bias_leaky'):
        assert stored_ratio(F.fwd_by_slices(name, mode, e, n, bias_each=True), name, mode, e) > 1.0, e


@pytest.mark.parametrize('name,mode', SLICED)
def test_mutation_leaky_applied_per_slice(ops, name, mode):
    n = slices_of(ops, name, mode)
    assert stored_ratio(F.fwd_by_slices(name, mode, 'bias_leaky', n, leaky_each=True), name, mode, 'bias_leaky') > 1.0


@pytest.mark.parametrize('name,mode,epilogue', [c for c in FWD if c[1] == 'bf16'])
def test_mutation_bf16_store_truncates(name, mode, epilogue):
    ref = F.fwd_reference(name, mode, epilogue)['y']
    assert F.bf16_ratio(F.stored(ref, mode), ref) <= 1.0
    assert F.bf16_ratio(F.stored(ref, mode, F.bf16_truncate), ref) > 1.0


@pytest.mark.parametrize('name,mode,epilogue', FWD)
def test_mutation_one_row_too_many(name, mode, epilogue):
    assert stored_ratio(F.fwd_by_slices(name, mode, epilogue, 1, extra_row=True), name, mode, epilogue) > 1.0


@pytest.mark.parametrize('name,mode', WGRAD)
def test_mutation_filter_gradient_pixels(name, mode):
    c, ref = F.wgrad_case(name), F.wgrad_reference(name, mode)
    B = c['B']
    missing = F.wgrad_of(c, mode, pixels=range(B - 1)).astype(np.float32)
    assert F.wgrad_ratio(missing, ref, mode) > 1.0
    if B >= 2:
        twice = F.wgrad_of(c, mode, pixels=list(range(B)) + [0]).astype(np.float32)
        assert F.wgrad_ratio(twice, ref, mode) > 1.0
        assert F.wgrad_ratio(F.wgrad_of(c, mode, pixels=range(B)).astype(np.float32), ref, mode) <= 1.0
