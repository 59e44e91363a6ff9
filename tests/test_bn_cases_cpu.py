"""The batch-norm cases of tests/bn_cases.py, checked without a GPU: the launch geometry restated from the kernels covers every (row, channel
group) exactly once and reaches every loop part; every lattice input is one on which a correct kernel and the float64 oracle must agree
(no |z| near 0 that is not exactly 0, no near-tie of a pool window's two best activations); an f32 restatement of the kernels' arithmetic
fits every bound of tests/test_bn_gpu.py; and each of twelve mistakes a kernel could make breaks a bound or an exact assertion in a
named case (the mutations at the end)."""
import numpy as np
import pytest

import bn_cases as B
from oracle import yolo2_ref as R

f32 = np.float32


def _geometry_runs():
    """(kernel, rows, C, vec) of every launch of groups A, B and C: `rows` is M, or the pooled pixel count for the pooled kernels."""
    runs = set()
    shapes = [(B.LATTICE[n][:3], B.LATTICE[n][3], m) for n, m in B.LATTICE_RUNS]
    shapes += [(B.POOL_SHAPE_OF_M.get(M, (1, M, 1)), C, m) for M, C in B.STATS_SHAPES for m in B.MODES]
    for (b, h, w), C, mode in shapes:
        for kernel in B.KERNELS:
            pooled = 'pool' in kernel
            if pooled and (h % 2 or w % 2):
                continue
            runs.add((kernel, b * (h // 2) * (w // 2) if pooled else b * h * w, C, B.VEC[mode]))
    return sorted(runs)


GEOMETRY = _geometry_runs()


def test_rowmap_covers_every_row_and_channel_group_exactly_once():
    """RowMap (tpr, rpp, cg, rs, active), colsum_grid and rowmap_grid are RESTATED in bn_cases.py from csrc/colsum.h and csrc/bn.hip.  For every
    launch of the GPU file: the active threads of all workgroups touch each (row, channel group) exactly once, no active thread's vector
    ends beyond C, and no row >= the row count is read."""
    for kernel, rows, C, vec in GEOMETRY:
        grid = B.KERNELS[kernel][0](rows, C, vec)
        visits, top_channel, top_row = B.coverage(rows, C, vec, grid)
        assert visits.shape == (rows, C // vec) and np.all(visits == 1), (kernel, rows, C, vec, grid)
        assert top_channel <= C and top_row == rows - 1, (kernel, rows, C, vec, top_channel, top_row)
        rm = B.RowMap(C, vec)
        assert rm.active.sum() == rm.tpr * rm.rpp <= 256 and rm.cg[rm.active].max() == rm.tpr - 1


def test_geometry_reaches_every_loop_part_and_every_threads_per_row():
    seen = {k: [False, False, False, False] for k in B.KERNELS}
    for kernel, rows, C, vec in GEOMETRY:
        grid = B.KERNELS[kernel][0](rows, C, vec)
        unrolled, tail, ragged = B.loop_profile(rows, C, vec, grid)
        several = bool(B.rows_per_thread(rows, C, vec, grid).max() > 1)
        for i, v in enumerate((unrolled, tail, ragged, several)):
            seen[kernel][i] |= v
    for kernel, (grid_rule, has_unrolled) in B.KERNELS.items():
        unrolled, tail, ragged, several = seen[kernel]
        assert ragged and several, kernel                                   # a ragged last step, and a loop that runs more than once
        if has_unrolled:
            assert unrolled and tail, kernel                                # the four-way unrolled loop and the single-row loop behind it
    assert {1, 2, 3, 5, 6, 12, 24, 40, 65, 128, 256} <= {C // vec for _, _, C, vec in GEOMETRY}
    # idle threads: threads-per-row values that do not divide 256 leave 256 - tpr * rpp of them
    assert any(B.RowMap(C, vec).active.sum() < 256 for _, _, C, vec in GEOMETRY)
    # c of the bounds, written next to the cases: the smallest and the largest in use
    cs = sorted({B.chain_terms(rows, C, vec) for kernel, rows, C, vec in GEOMETRY if B.KERNELS[kernel][0](rows, C, vec) == B.colsum_grid(rows, C, vec)})
    print('chain terms c in use: %d .. %d' % (cs[0], cs[-1]))
    assert cs[0] >= 4 and cs[-1] <= 6 + 256 + 2


def test_fin_supported_restates_the_library_rule():
    for C in B.CHANNELS:
        for mode in B.channel_modes(C):
            tpr = C // B.VEC[mode]
            assert B.fin_supported(16, C, B.VEC[mode]) == (tpr & (tpr - 1) == 0)
    assert not B.fin_supported(256, 1024, 8) and B.fin_supported(256, 1024, 4) and B.fin_supported(128, 1024, 8)      # rows x slice x 8 bytes <= 128 KB


def test_shift_distance_table():
    """The table of the docstring of bn_cases.py and of profiles/bn_cases.md."""
    want = {1: 23.6, 10: 7.5, 27: 4.5, 134: 2.0, 340: 1.1, 678: 0.70}
    assert B.chain_terms(2704, 1024, 8) == 10 and B.chain_terms(1352, 96, 8) == 27 and B.chain_terms(2704, 8, 4) == 134
    for c, k in want.items():
        assert abs(B.shift_distance(c) - k) <= 0.06, (c, B.shift_distance(c))


def test_bwd_apply64_is_the_oracles_backward_when_the_sums_are_the_batchs_own():
    c = B.lattice_case('d_8x6_40', 'f32')
    y, da = c['y'].astype(np.float64), c['da'].astype(np.float64)
    par = [c[k].astype(np.float64) for k in ('mean', 'var', 'gamma', 'beta')]
    z, _ = B.fwd64(y, *par)
    dx, dgamma, dbeta = R.bn_train_bwd(y, par[0], par[1], par[2], R.leaky_relu_grad(z, da, B.ALPHA), B.EPS)
    g, gx = B.bwd_terms64(y, da, *par)
    np.testing.assert_allclose(gx.reshape(-1, c['C']).sum(0), dgamma, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g.reshape(-1, c['C']).sum(0), dbeta, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(B.bwd_apply64(y, da, *par, dgamma, dbeta, c['M']), dx, rtol=1e-11, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# B and C: conditions of the inputs, and the restatement inside the bounds
# ---------------------------------------------------------------------------------------------------------------------

def lattice_check(name, mode, mut=None):
    """The f32 restatement of every kernel on a lattice case against the float64 references.  -> (ratios: output -> worst |err| / bound,
    exact: assertion -> bool)."""
    c, ref = B.lattice_case(name, mode), B.lattice_reference(name, mode)
    M, C, vec = c['M'], c['C'], B.VEC[mode]
    par = (c['mean'], c['var'], c['gamma'], c['beta'])
    y = c['y']
    ratios, exact = {}, {}
    z32, a32 = B.fwd32(y, *par, mut)
    a_st = B.store32(a32, mode, mut)
    ratios['a'] = B.grad_ratio(a_st, ref['a'], mode)
    exact['a is 0 where z is 0'] = bool(np.all(a_st[ref['z'] == 0] == 0))
    g, xh = B.bwd_terms32(y, c['da'], *par, mut)
    grid = B.colsum_grid(M, C, vec)
    ct = B.chain_terms(M, C, vec)
    sums = lambda t, gr: B.chain_sums32(t.reshape(-1, C), C, vec, gr).astype(np.float64).sum(0).astype(f32)
    ratios['dgamma'] = float(B.reduced_ratio(sums(g * xh, grid), ref['gx'], ct).max())
    ratios['dbeta'] = float(B.reduced_ratio(sums(g, grid), ref['g'], ct).max())
    dy = B.store32(B.bwd_apply32(y, c['da'], *par, c['dgamma_in'], c['dbeta_in'], M, mut), mode, mut)
    ratios['dy'] = B.grad_ratio(dy, ref['dy'], mode)
    y2 = y.reshape(M, C)
    mean, var = B.stats32(y2, y2[0], C, vec, grid, mut)
    rm, rv = B.moment_ratios(mean, var, y2, y2[0], ct)
    ratios['mean'], ratios['var'] = float(rm.max()), float(rv.max())
    exact['var >= 0'] = bool(np.all(var >= 0))
    if c['pooled']:
        MP = M // 4
        arg, p = B.pool32(a_st, a32, mode, mut)
        exact['arg-max'] = bool(np.array_equal(arg, ref['arg']))
        ratios['p'] = B.grad_ratio(p, ref['p'], mode)
        ymax = B.take(B.windows(y), arg)
        exact['ymax'] = bool(np.array_equal(ymax, ref['ymax']))
        pgrid, pct = B.colsum_grid(MP, C, vec), B.chain_terms(MP, C, vec)
        pg, pxh = B.bwd_terms32(ymax, c['dp'], *par, mut)
        ratios['pooled dgamma'] = float(B.reduced_ratio(sums(pg * pxh, pgrid), ref['pgx'], pct).max())
        ratios['pooled dbeta'] = float(B.reduced_ratio(sums(pg, pgrid), ref['pg'], pct).max())
        pdy = B.bwd_apply32(y, B.route(c['dp'], arg).astype(f32), *par, c['dgamma_in'], c['dbeta_in'], MP if mut == 'pooled_count' else M, mut)
        ratios['pooled dy'] = B.grad_ratio(B.store32(pdy, mode, mut), ref['pdy'], mode)
    return ratios, exact


def passes(ratios, exact):
    return all(r <= 1.0 for r in ratios.values()) and all(exact.values())


@pytest.mark.parametrize('name,mode', B.LATTICE_RUNS)
def test_lattice_case_conditions_and_restatement(name, mode):
    c, ref = B.lattice_case(name, mode), B.lattice_reference(name, mode)
    assert all(np.all(np.isfinite(v)) for v in ref.values())
    assert np.array_equal(c['y'], B.inputs64(c['y'], mode)) and np.array_equal(c['da'], B.inputs64(c['da'], mode))       # exact in bf16
    cond = B.conditions(name, mode)
    print(name, mode, cond)
    # EVERY element: |z| is exactly 0 or at least MARGIN of the channel's largest; EVERY window: the two best activations are bit-equal after
    # the store's rounding or at least the threshold apart
    assert cond['zmargin'] >= B.MARGIN, cond
    assert cond['zeros'] > 0
    if c['pooled']:
        assert cond['gap'] >= 1.0, cond
    if c['C'] >= 16:
        assert cond['neg_zero'] > 0                                          # -0.0: a channel with beta 0 and a negative gamma
    assert (c['gamma'] < 0).sum() == c['C'] // 5
    if name in B.DECISION_CASES:
        assert all(n >= 2 for n in c['planted'].values()), c['planted']
        for kind in B.WINDOW_KINDS:
            assert cond[kind] >= c['planted'][kind], (kind, cond)
        assert (cond['collision'] > 0) == (mode == 'bf16'), cond
    # the rows test_bn_gpu.py hands the *_fin consumers finalise to exactly the case's mean and var, for every row count
    for rows in B.FIN_ROWS:
        mean, var = B.rows_moments(B.exact_rows(c['fin_s2'], rows), rows, c['mean'], c['M'])
        assert np.array_equal(mean, c['mean']) and np.array_equal(var, c['var']) and np.all(var > 0)
    ratios, exact = lattice_check(name, mode)
    print(name, mode, {k: round(v, 3) for k, v in ratios.items()})
    assert passes(ratios, exact), (ratios, exact)


# ---------------------------------------------------------------------------------------------------------------------
# A: statistics conditioning
# ---------------------------------------------------------------------------------------------------------------------

def stats_check(M, C, mode, mut=None):
    """bn_stats restated (first-sample shift, f32 chains) and the host-built rows of every (placement, rows) pair of the shape, finalised as
    the kernels do.  -> (ratios, exact)."""
    c = B.stats_case(M, C, mode)
    y, vec = c['y'], B.VEC[mode]
    ratios, exact = {}, {}
    mean, var = B.stats32(y, y[0], C, vec, B.colsum_grid(M, C, vec), mut)
    rm, rv = B.moment_ratios(mean, var, y, y[0], B.chain_terms(M, C, vec))
    ratios['bn_stats mean'], ratios['bn_stats var'] = float(rm.max()), float(rv.max())
    exact['bn_stats var >= 0'] = bool(np.all(var >= 0))
    const = c['kind'] == B.KIND_CONST
    exact['bn_stats constant channels'] = bool(np.all(var[const] == 0) and np.array_equal(mean[const], y[0, const]))
    for placement, rows in B.fin_combos(M, C):
        shift = B.placed_shift(y, placement)
        mean, var = B.rows_moments(B.host_rows(y, shift, rows), rows, shift, M, mut)
        rm, rv = B.moment_ratios(mean, var, y, shift, 1)
        ratios['rows %s/%d mean' % (placement, rows)], ratios['rows %s/%d var' % (placement, rows)] = float(rm.max()), float(rv.max())
        exact['rows %s/%d var >= 0' % (placement, rows)] = bool(np.all(var >= 0))
        if placement == 'mean':
            assert np.array_equal(shift[const], y[0, const])
            exact['rows constant channels'] = bool(np.all(var[const] == 0) and np.array_equal(mean[const], y[0, const]))
            _, a = B.fwd32(y[:, const], mean[const], var[const], c['gamma'][const], c['beta'][const], mut)
            exact['constant channels give leaky(beta)'] = bool(np.all(a == np.maximum(c['beta'][const], f32(B.ALPHA) * c['beta'][const])))
    return ratios, exact


@pytest.mark.parametrize('mode', B.MODES)
@pytest.mark.parametrize('M,C', B.STATS_SHAPES)
def test_stats_case_and_restatement(M, C, mode):
    c = B.stats_case(M, C, mode)
    y64 = c['y'].astype(np.float64)
    assert np.all(np.isfinite(y64)) and np.array_equal(c['y'], B.inputs64(c['y'], mode))
    assert set(c['kind'].tolist()) == set(range(8))
    const = c['kind'] == B.KIND_CONST
    assert np.all(y64[:, const].var(0) == 0)
    if mode == 'f32' and M >= 105:
        r = np.abs(y64.mean(0)) / y64.std(0).clip(1e-30)
        for k, want in enumerate(B.RATIOS[1:], 1):
            assert np.all(np.abs(r[c['kind'] == k] / want - 1) < 0.5), k            # mean / std ratios 3 .. 3000 side by side
        assert np.all(y64[:, c['kind'] == B.KIND_OUTLIER].max(0) == 1000)
    ratios, exact = stats_check(M, C, mode)
    print(M, C, mode, {k: round(v, 3) for k, v in ratios.items()})
    assert passes(ratios, exact), (ratios, exact)


def test_placements_and_rows_pair_up_completely():
    pairs = {p for M, C in B.STATS_SHAPES for p in B.fin_combos(M, C)}
    assert pairs == {(p, r) for p in B.PLACEMENTS for r in B.FIN_ROWS}
    for M, C in B.STATS_SHAPES:
        assert [p for p, _ in B.fin_combos(M, C)] == list(B.PLACEMENTS)


def test_variance_bound_needs_the_mean_planes_term():
    """A bound of the form 1e-5 var + c u E2 is missed by CORRECT code: one exactly summed, once rounded row per plane (rows = 1, c = 1) with the
    shift 300 std away.  var = E2 - dm^2: rounding the sum plane by r1 u and the square plane by r2 u moves the variance by
    u (r2 E2 - 2 r1 dm^2) ~ u E2 (r2 - 2 r1), up to 3 u E2.  With the term 2 |dm| E1 the same rows fit."""
    worst_issue, worst = 0.0, 0.0
    for M, C in B.STATS_SHAPES:
        y = B.stats_case(M, C, 'f32')['y']
        shift = B.placed_shift(y, '300std')
        mean, var = B.rows_moments(B.host_rows(y, shift, 1), 1, shift, M)
        worst_issue = max(worst_issue, float(B.moment_ratios(mean, var, y, shift, 1, issue_form=True)[1].max()))
        worst = max(worst, float(B.moment_ratios(mean, var, y, shift, 1)[1].max()))
    print('one rounded row, shift 300 std away: worst |err| / bound %.2f without the term, %.2f with it' % (worst_issue, worst))
    assert worst_issue > 1.0 and worst <= 1.0


def test_conv_cases():
    for shape in B.CONV_SHAPES:
        for k in B.CONV_KSIZES:
            c = B.conv_case(shape, k)
            y = R.conv2d(c['x'].astype(np.float64), c['w'].astype(np.float64)).reshape(-1, shape[4])
            assert np.all(np.abs(y.mean(0) - c['means']) < 0.5) and np.all(np.abs(y.std(0) - 1) < 0.5)      # the chosen means, std ~ 1
            assert set(np.abs(c['means']).tolist()) == set(B.CONV_MEANS) and np.all(c['x'][..., 0] == 1)


# ---------------------------------------------------------------------------------------------------------------------
# D: moving averages
# ---------------------------------------------------------------------------------------------------------------------

def test_ema_restatement():
    rng = np.random.RandomState(5)
    m, x = rng.randn(64).astype(f32) * 3, rng.randn(64).astype(f32)
    for decay in B.EMA_DECAYS:
        plain, fused = B.ema32(m, x, decay)
        exact = m.astype(np.float64) - (m.astype(np.float64) - x.astype(np.float64)) * float(f32(1.0 - decay))
        assert np.all(np.abs(plain - exact) <= 2.0 ** -22 * np.abs(m)) and np.all(np.abs(fused - exact) <= 2.0 ** -22 * np.abs(m))
        assert np.array_equal(B.ema32(m, m, decay)[0], m) and np.array_equal(B.ema32(m, m, decay)[1], m)       # moving == batch: unchanged
        assert np.array_equal(plain, R.bn_ema(m, x, decay))
    assert B._round_f32(B.fractions.Fraction(1) + B.fractions.Fraction(1, 2 ** 24)) == f32(1)                  # a tie goes to even
    assert B._round_f32(B.fractions.Fraction(1) + B.fractions.Fraction(3, 2 ** 24)) == f32(1) + f32(2.0 ** -22)


# ---------------------------------------------------------------------------------------------------------------------
# mutation proofs: mistake -> the named case whose bound or exact assertion it breaks
# ---------------------------------------------------------------------------------------------------------------------

def ema_check(mut=None):
    rng = np.random.RandomState(6)
    m, x = rng.randn(32).astype(f32) * 3, rng.randn(32).astype(f32)
    return {}, {'ema %g' % d: B.ema_matches(B.ema32(m, x, d)[0], m, x, d, mut) for d in B.EMA_DECAYS}


CAUGHT_BY = {
    'unshifted':            lambda mut: stats_check(676, 32, 'f32', mut),
    'shift_sum_plane_only': lambda mut: stats_check(676, 32, 'f32', mut),
    'unbiased':             lambda mut: stats_check(4, 8, 'f32', mut),
    'eps_outside_sqrt':     lambda mut: lattice_check('d_8x6_40', 'f32', mut),
    'z_gt_0':               lambda mut: lattice_check('d_8x6_40', 'f32', mut),
    'sign_of_y_minus_mean': lambda mut: lattice_check('d_8x6_40', 'f32', mut),
    'truncating_store':     lambda mut: lattice_check('d_8x6_40', 'bf16', mut),
    'last_max':             lambda mut: lattice_check('d_8x6_40', 'f32', mut),
    'argmax_unrounded':     lambda mut: lattice_check('d_8x6_40', 'bf16', mut),
    'pooled_count':         lambda mut: lattice_check('d_8x6_40', 'f32', mut),
    'decay_swapped':        lambda mut: ema_check(mut),
    'no_clamp':             lambda mut: stats_check(2704, 32, 'f32', mut),
}
EVERYWHERE = [lambda mut: stats_check(676, 32, 'f32', mut), lambda mut: stats_check(4, 8, 'f32', mut), lambda mut: stats_check(2704, 32, 'f32', mut),
              lambda mut: lattice_check('d_8x6_40', 'f32', mut), lambda mut: lattice_check('d_8x6_40', 'bf16', mut), ema_check]


@pytest.mark.parametrize('mut', B.MUTATIONS)
def test_mutation_is_caught_by_its_named_case(mut):
    assert set(CAUGHT_BY) == set(B.MUTATIONS)
    ratios, exact = CAUGHT_BY[mut](None)
    assert passes(ratios, exact)                                              # the case itself passes
    ratios, exact = CAUGHT_BY[mut](mut)
    broken = sorted([k for k, v in ratios.items() if not v <= 1.0] + [k for k, v in exact.items() if not v])
    print(mut, '->', broken)
    assert broken, mut


@pytest.mark.parametrize('mut', B.MUTATIONS)
def test_no_mutation_passes_everywhere(mut):
    assert not all(passes(*check(mut)) for check in EVERYWHERE), mut
