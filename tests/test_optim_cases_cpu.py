"""The optimizer, clip and arena-kernel cases of tests/optim_cases.py, checked without a GPU: `step` restates the oracle bit for bit; the f32
oracle stays inside every bound of tests/test_optim_gpu.py against the float64 reference on every case (the worst ratio per group is
printed); the cases contain what they claim (exact zeros, squares that underflow, sqrt(v) ~ eps, Ftrl's planted decisions computed without
rounding and every other element away from l1, every branch of zero_ranges_kernel); and each of ten faults planted into the f32 oracle
leaves at least one bound on at least one case."""
import numpy as np
import pytest

import optim_cases as O

f32 = np.float32
CHAINS = [(name, n, gs) for name in O.CONFIGS for n in O.SIZES for gs in O.GSCALES]


def _worst(chains, mut=None):
    """{config name: {output: worst ratio}} of the f32 oracle (with a planted fault) over `chains`."""
    out = {}
    for name, n, gs in chains:
        w = O.run_chain(name, n, gs, O.oracle32_stepper(mut), mut=mut)
        d = out.setdefault(name, {})
        for k, v in w.items():
            d[k] = min(d.get(k, np.inf), v) if k == 'decision_distance' else max(d.get(k, 0.0), v)
    return out


def _breaks(worst):
    return {(n, k): v for n, d in worst.items() for k, v in d.items() if k != 'decision_distance' and not v <= 1}


def test_step_restates_the_oracle_bit_for_bit():
    """In f32 and in f64, on hyper-parameters that are f32 numbers (0.5, 0.75, 2^-20 ...): there the oracle's own conversions are the ABI's, and
    its alpha is optim.py's."""
    hps = {'adam': {'beta1': 0.5, 'beta2': 0.75, 'epsilon': 2.0 ** -27}, 'momentum': {'momentum': 0.875}, 'gd': {},
           'rmsprop': {'decay': 0.875, 'momentum': 0.5, 'epsilon': 2.0 ** -33}, 'adagrad': {}, 'adadelta': {'rho': 0.9375, 'epsilon': 2.0 ** -27},
           'ftrl': {'learning_rate_power': -0.5, 'l1_regularization_strength': 0.0625, 'l2_regularization_strength': 0.015625}}
    lr, n, gs = 2.0 ** -7, 1025, 1.0 / 3
    for kind, hp in hps.items():
        for power in ((-0.5, -0.75) if kind == 'ftrl' else (None,)):
            if power is not None:
                hp = dict(hp, learning_rate_power=power)
            rng = np.random.RandomState(3)
            state32 = (rng.randn(n).astype(f32),) + tuple((0.1 + rng.rand(n)).astype(f32) for _ in O.SLOTS[kind])
            g = rng.randn(n).astype(f32)
            for ty in (f32, np.float64):
                state = tuple(x.astype(ty) for x in state32)
                # t = 1: sqrt(1 - 0.75) / (1 - 0.5) = 1, so alpha = lr is an f32 number and the oracle's float64 alpha is the ABI's
                alpha = O.alpha_of(hp, lr, 1) if kind == 'adam' else None
                assert alpha is None or alpha == lr
                mine = O.step(kind, hp, state, g, gs, ty, lr=lr, alpha=alpha)
                theirs = O.oracle_step(kind, hp, state, O.scaled(g, gs).astype(ty), lr, 1)
                for a, b in zip(mine, theirs):
                    assert a.dtype == ty and np.array_equal(a, b), (kind, power, ty)


def test_f32_oracle_fits_every_bound_on_every_case(capsys):
    worst = _worst(CHAINS)
    with capsys.disabled():
        for name, d in worst.items():
            print('f32 oracle, %-16s worst |err| / bound: %s' % (name + ':', '  '.join('%s %.3f' % kv for kv in sorted(d.items()))))
    assert not _breaks(worst), _breaks(worst)
    for name, d in worst.items():
        if 'decision_distance' in d and O.F(O.CONFIGS[name][2]['l1_regularization_strength']) > 0:
            assert d['decision_distance'] >= 2, (name, d)


def test_cases_contain_what_they_claim():
    for gs in O.GSCALES:
        i = np.arange(10007)
        for t in (1, 7):
            g = O.gradient('adam', 10007, gs, t)
            gi = O.scaled(g, gs)
            assert np.all(g[i % 16 == O.ZERO_AT] == 0)
            under = gi[i % 16 == O.UNDERFLOW_AT]
            assert np.all(under != 0) and np.all(under * under == 0)                      # the square underflows, the element does not
            rest = np.abs(g[~np.isin(i % 16, (O.ZERO_AT, O.UNDERFLOW_AT, O.NEAR_EPS_AT))])
            assert rest.min() < 1e-9 and rest.max() > 10 and rest.min() >= 0.99e-10 and rest.max() <= 1.01e2
            assert (g < 0).any() and (g > 0).any()
    # Adam: sqrt(v) within a factor of ten of eps in the NEAR_EPS_AT elements, at some step of every gradient scale
    kind, lr, hp = O.CONFIGS['adam']
    for gs in O.GSCALES:
        state, seen = O.init_state('adam', 10007, gs), False
        for t in range(1, O.T + 1):
            state = O.step(kind, hp, state, O.gradient('adam', 10007, gs, t), gs, f32, alpha=O.alpha_of(hp, lr, t))
            r = np.sqrt(state[2][np.arange(10007) % 16 == O.NEAR_EPS_AT]) / O.F(hp['epsilon'])
            seen |= bool(np.all((r > 0.1) & (r < 10)))
        assert seen
    # Ftrl: the planted elements are computed without rounding, and sit on l1, one f32 below and one f32 above
    for name in ('ftrl_sqrt_l1_l2', 'ftrl_pow_l1'):
        kind, lr, hp = O.CONFIGS[name]
        l1 = f32(hp['l1_regularization_strength'])
        for gs in O.GSCALES:
            for n in (255, 10007):
                state = O.init_state(name, n, gs)
                g = O.settle(name, state, O.gradient(name, n, gs, 1), gs, lr)
                assert np.array_equal(g, O.gradient(name, n, gs, 1)) or n == 10007       # (settle moves few elements, and no planted one)
                new32, new64 = O.step(kind, hp, state, g, gs, f32, lr=lr), O.step(kind, hp, state, g, gs, np.float64, lr=lr)
                i = np.arange(n)
                for k, want, zero in zip(O.PLANT_AT, (l1, np.nextafter(l1, f32(0)), np.nextafter(l1, f32(np.inf))), (True, True, False)):
                    sel = i % 16 == k
                    assert sel.any() and np.all(np.abs(new32[2][sel]) == want) and np.array_equal(new32[2][sel].astype(np.float64), new64[2][sel])
                    assert np.all((new32[0][sel] == 0) == zero) and np.all((new64[0][sel] == 0) == zero)
                assert np.isinf(O.bounds(kind, hp, state, g, gs, lr=lr)['decision'][np.isin(i % 16, O.PLANT_AT)]).all()
    # Ftrl with l1 = l2 = 0: the 0 / 0 elements
    kind, lr, hp = O.CONFIGS['ftrl_sqrt']
    state = O.init_state('ftrl_sqrt', 1025, 1.0)
    sel = np.arange(1025) % 32 == O.ZERO_AT
    new = O.step(kind, hp, state, O.gradient('ftrl_sqrt', 1025, 1.0, 1), 1.0, f32, lr=lr)
    assert np.all(state[1][sel] == 0) and np.all(new[1][sel] == 0) and np.all(new[0][sel] == 0) and np.all(new[2][sel] == 0)


MUTATION_CHAINS = {
    'adam_eps_in_sqrt': [('adam', 1025, 1.0 / 8)],
    'adam_t_off_by_one': [('adam', 255, 1.0)],
    'gscale_after_square': [(name, 1023, 1.0 / 3) for name in ('adam', 'rmsprop', 'adagrad', 'adadelta', 'ftrl_sqrt')],
    'adadelta_updated_accu': [('adadelta', 1024, 1.0)],
    'rmsprop_eps_outside_sqrt': [('rmsprop', 1025, 1.0 / 3)],
    'momentum_lr_on_g': [('momentum', 5, 1.0)],
    'ftrl_ge': [('ftrl_sqrt', 255, 1.0)],
}


@pytest.mark.parametrize('mut', sorted(MUTATION_CHAINS))
def test_planted_fault_leaves_a_bound(mut):
    chains = MUTATION_CHAINS[mut]
    assert not _breaks(_worst(chains)), 'the unmutated f32 oracle must pass the same chains'
    broken = _breaks(_worst(chains, mut))
    print(mut, broken)
    assert broken
    if mut == 'gscale_after_square':
        assert {n for n, _ in broken} == {n for n, _, _ in chains}           # caught in every optimizer that squares the gradient


def test_every_listed_fault_is_planted_somewhere():
    planted = set(MUTATION_CHAINS) | {'clip_f32_sum', 'clip_nan_ignored', 'zero_ranges_a_down'}
    assert planted == set(O.MUTATIONS) and len(planted) == 10


def test_gscale_of_one_hides_the_square_fault():
    """Why the gradient scales 1/3 and 1/8 are there: with gscale = 1 the fault is invisible."""
    assert not _breaks(_worst([('adam', 1023, 1.0)], 'gscale_after_square'))


# ------------------------------------------------------------------------------------------------------------------
# clip
# ------------------------------------------------------------------------------------------------------------------

def test_clip_table_holds_every_length_and_content():
    assert {n for n, _ in O.CLIP_TABLE} == {0, 1, 63, 64, 65, 257, 64 * 256 + 7, 70001}
    assert {c for _, c in O.CLIP_TABLE} == {'empty', 'zeros', 'below', 'eq_clip', 'big', 'overflow', 'tiny'}
    c = O.clip_case('full_table')
    for s, content in enumerate(c['contents']):
        x = c['g'][c['seg_off'][s]:c['seg_off'][s + 1]]
        norm = np.sqrt((x.astype(np.float64) ** 2).sum())
        with np.errstate(over='ignore', under='ignore'):
            sq32 = x * x
        if content in ('below', 'tiny', 'zeros', 'empty'):
            assert norm < 2e-3 * O.CLIP
        if content == 'eq_clip':
            assert norm == O.CLIP and (x != 0).sum() == 1
        if content == 'big':
            assert abs(norm / (1e4 * O.CLIP) - 1) < 1e-6
        if content == 'overflow':
            assert np.isinf(sq32).all() and np.isfinite(norm) and norm > O.CLIP
        if content == 'tiny':
            assert np.all(x != 0) and np.all(sq32 == 0)
    n = O.clip_case('non_finite')
    assert n['contents'] == ['big', 'inf', 'below', 'nan', 'big'] and np.isinf(n['g']).sum() == 1 and np.isnan(n['g']).sum() == 1


@pytest.mark.parametrize('name', sorted(O.CLIP_CASES))
def test_f32_clip_model_fits_the_bound(name, capsys):
    c = O.clip_case(name)
    got = O.clip_model32(c['g'], c['seg_off'], O.CLIP)
    worst, bad = O.clip_check(got, c['g'], c['seg_off'], O.CLIP)
    with capsys.disabled():
        print('f32 clip model, %s: worst |err| / (5 u |ref|) = %.3f' % (name, worst))
    assert not bad, bad
    again = O.clip_model32(got, c['seg_off'], O.CLIP)          # a second clip of a clipped gradient: the norm is clip up to rounding
    assert not O.clip_check(again, got, c['seg_off'], O.CLIP)[1]


@pytest.mark.parametrize('mut,name', [('clip_f32_sum', 'full_table'), ('clip_nan_ignored', 'non_finite')])
def test_planted_clip_fault_is_caught(mut, name):
    c = O.clip_case(name)
    _, bad = O.clip_check(O.clip_model32(c['g'], c['seg_off'], O.CLIP, mut), c['g'], c['seg_off'], O.CLIP)
    print(bad)
    assert bad
    if mut == 'clip_f32_sum':
        assert {c['contents'][int(b.split()[1])] for b in bad} == {'overflow'}


# ------------------------------------------------------------------------------------------------------------------
# zero_ranges, bn_fold
# ------------------------------------------------------------------------------------------------------------------

def test_zero_ranges_cases_reach_every_branch():
    cases = O.zero_ranges_cases()
    seen_pairs = set()
    for name, (n, ranges) in cases.items():
        assert all(0 <= a <= b <= n for a, b in ranges), name
        flat = sorted(ranges)
        assert all(b0 <= a1 for (_, b0), (a1, _) in zip(flat[:-1], flat[1:])), name          # disjoint: 'outside' is well defined
        seen_pairs |= {(a % 4, b % 4, b - a) for a, b in ranges}
    assert {(a, (a + ln) % 4, ln) for a in range(4) for ln in range(10)} <= seen_pairs
    br = {name: O.zero_ranges_branches(r) for name, (_, r) in cases.items()}
    assert br['short_branch'] == (True, False, False, False, 1)
    assert br['scalar_edges_long'][:4] == (False, True, True, True)
    assert br['multi_launch_17_ranges'][4] == 2 and br['multi_launch_33_ranges'][4] == 3 and br['every_a_mod_4_b_mod_4_lengths_0_to_9'][4] == 3
    assert any(b == n for n, r in cases.values() for _, b in r)                              # a range that runs to the end
    assert O.zero_ranges_branches(O.ZERO_RANGES_STRIDED[1])[1:4] == (True, True, True)
    assert (O.ZERO_RANGES_STRIDED[1][0][1] - O.ZERO_RANGES_STRIDED[1][0][0]) // 4 > 8192 * 256


def test_planted_zero_ranges_fault_is_caught():
    caught = []
    for name, (n, ranges) in O.zero_ranges_cases().items():
        x = np.full(n, O.SENTINEL, np.uint32)
        want = O.zero_ranges_model(x, ranges)
        inside = np.zeros(n, bool)
        for a, b in ranges:
            inside[a:b] = True
        assert np.all(want[inside] == 0) and np.all(want[~inside] == O.SENTINEL)
        if not np.array_equal(O.zero_ranges_model(x, ranges, 'zero_ranges_a_down'), want):
            caught.append(name)
    assert len(caught) >= 4, caught


@pytest.mark.parametrize('rows,C', O.BN_FOLD_SHAPES)
def test_f32_bn_fold_fits_the_bound(rows, C, capsys):
    case = O.bn_fold_case(rows, C)
    if C >= 32:
        assert (case['gamma'] < 0).any() and (case['gamma'] == 0).any() and (case['var'] == 0).any() and case['cancel'].any()
        rb = O.bn_fold_model(case, np.float64)[1]
        assert np.abs(rb[case['cancel']]).max() < 1e-6 * np.abs(case['beta'][case['cancel']]).max()       # beta - mean s cancels
    with np.errstate(all='ignore'):
        Wf, bias = O.bn_fold_model(case, f32)
    rw, rbias = O.bn_fold_check(Wf, bias, case)
    with capsys.disabled():
        print('f32 bn_fold %dx%d: worst |err| / bound: Wf %.3f bias %.3f' % (rows, C, rw, rbias))
    assert rw <= 1 and rbias <= 1
    # eps outside the root, and the bias from the unscaled mean, are caught
    s_bad = case['gamma'] / (np.sqrt(case['var']) + f32(O.F(O.BN_EPS)))
    if C >= 32:
        assert O.bn_fold_check(case['W'] * s_bad, bias, case)[0] > 1
        assert O.bn_fold_check(Wf, case['beta'] - case['mean'], case)[1] > 1


def test_scale_factors_round():
    """1/3 and 1e-3 are factors whose product is rounded (0.125, the factor of tests/test_kernels_gpu.py, is exact in any rounding mode)."""
    x = O.scale_input(10007)
    for s in (1.0 / 3, 1e-3):
        exact = x.astype(np.float64) * O.F(s)
        assert (exact != (x * f32(s)).astype(np.float64)).mean() > 0.5
