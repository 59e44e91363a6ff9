"""The batch-norm family (csrc/bn.hip, csrc/bn_stats.hip; arithmetic in csrc/bn_leaky.h, reductions in csrc/colsum.h) in f32 AND bf16 against
the float64 oracle on exactly the values the kernels read, on the cases of tests/bn_cases.py: statistics with the shift at the mean and
1, 30 and 300 std away over channels whose mean / std ratio goes up to 3000 (A), every admitted channel count around the threads-per-row
values that do not divide 256 (B), exact zeros of z, negative gamma and planted pool windows (C), moving averages (D).  The inputs' own
conditions, the restated launch geometry (every shape launched here is one whose coverage tests/test_bn_cases_cpu.py has checked) and the
proof that these bounds catch a subtly wrong kernel are in tests/test_bn_cases_cpu.py; the bounds are derived in bn_cases.py.

Every output buffer starts out filled with NaN (arg-max bytes with 9) and padding lanes (lda, ldp, ldda larger than C by one vector or by
16) must still hold it afterwards; padding lanes of INPUTS hold NaN as well, so a kernel that read them would show it.  Every test
launches all its kernels and synchronises once before reading back."""
import numpy as np
import pytest
import torch

import bn_cases as B
from test_kernels_gpu import dev, host, part_row_sums, WORST      # noqa: E402
from yolo_tf_amd._lib import HipKernelError

pytestmark = pytest.mark.gpu

TD = {'f32': torch.float32, 'bf16': torch.bfloat16}
f32 = np.float32
NAN = float('nan')
REFUSED = 'argument check failed'
STATS_RUNS = [(M, C, m) for M, C in B.STATS_SHAPES for m in B.MODES]
CONV_RUNS = [(s, k, p, m) for s in B.CONV_SHAPES for k in B.CONV_KSIZES for p in B.CONV_SHIFTS for m in B.MODES]


@pytest.fixture(scope='module')
def ops():
    from yolo_tf_amd import ops as _ops
    _ops._lib.load()
    assert torch.cuda.is_available()
    return _ops


def nans(n, dtype=torch.float32):
    return torch.full((int(n),), NAN, dtype=dtype, device='cuda')


def workspace(C):
    return torch.full((1026 * C + 64,), NAN, dtype=torch.float64, device='cuda')


def upload(x, mode, ld=None):
    """A tensor [..., C] on the device in the kernel's dtype, exactly (the cases are already rounded); with ld, rows padded to ld with NaN."""
    x = np.array(x, dtype=f32)       # (a writable copy: the cases are read-only)
    assert np.array_equal(x, B.inputs64(x, mode))
    if ld is not None:
        padded = np.full(x.shape[:-1] + (ld,), np.nan, f32)
        padded[..., :x.shape[-1]] = x
        x = padded
    return dev(x, TD[mode])


def unpad(t, rows, C, ld, what):
    """[rows, ld] device buffer -> [rows, C] float64; the padding lanes must still hold the NaN they were filled with."""
    a = host(t).astype(np.float64).reshape(rows, ld)
    assert np.isnan(a[:, C:]).all(), '%s: padding lanes were written' % what
    assert not np.isnan(a[:, :C]).any(), '%s: elements left unwritten' % what
    return a[:, :C]


def ld_of(C, mode):
    """Leading dimension of the padded buffers: C + 16 or C + one vector, alternating over the channel counts."""
    return C + (16 if (C // 8) % 2 else B.VEC[mode])


def report(what, ratios, exact=()):
    for k, v in ratios.items():
        WORST['%s %s' % (what, k)] = float(v)
    print('%s: worst |err| / bound: %s' % (what, ', '.join('%s %.3f' % (k, v) for k, v in ratios.items())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (what, bad)
    failed = [k for k, v in dict(exact).items() if not v]
    assert not failed, (what, failed)


def moments(what, mean, var, y, shift, c, ratios, exact):
    m, v = host(mean), host(var)
    exact[what + ' finite, var >= 0'] = bool(np.all(np.isfinite(m)) and np.all(np.isfinite(v)) and np.all(v >= 0))
    rm, rv = B.moment_ratios(m, v, y, shift, c)
    ratios[what + ' mean'], ratios[what + ' var'] = float(rm.max()), float(rv.max())
    return m, v


def fin_agrees(ops, rows, C, mode):
    yes = ops.bn_fin_supported(rows, C, TD[mode])
    assert yes == B.fin_supported(rows, C, B.VEC[mode]), (rows, C, mode)
    return yes


# ---------------------------------------------------------------------------------------------------------------------
# A. statistics conditioning
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('M,C,mode', STATS_RUNS)
def test_bn_stats_conditioning(ops, M, C, mode):
    """bn_stats / bn_stats_ema: shift = the channel's first sample; c = chain_terms (rows per thread + rpp + 2).  The fused moving-average
    update with every decay, on moving values far from the batch's (30 std away) and, in every second channel, EQUAL to them."""
    c = B.stats_case(M, C, mode)
    y = c['y']
    yd, ws = upload(y, mode), workspace(C)
    mean, var = nans(C), nans(C)
    ops.bn_stats(yd, mean, var, ws, M, C)
    far_m, far_v = B.placed_shift(y, '30std'), (y.astype(np.float64).var(0) * 3 + 1).astype(f32)
    even = dev((np.arange(C) % 2 == 0)).bool()
    runs = []
    for decay in B.EMA_DECAYS:
        mm0, mv0 = torch.where(even, mean, dev(far_m)), torch.where(even, var, dev(far_v))      # (on the device: nothing is read back yet)
        mm, mv, mean2, var2 = mm0.clone(), mv0.clone(), nans(C), nans(C)
        ops.bn_stats_ema(yd, mean2, var2, mm, mv, decay, workspace(C), M, C)
        runs.append((decay, mm0, mv0, mm, mv, mean2, var2))
    torch.cuda.synchronize()
    ratios, exact = {}, {}
    ct = B.chain_terms(M, C, B.VEC[mode])
    m, v = moments('bn_stats (c = %d)' % ct, mean, var, y, y[0], ct, ratios, exact)
    const = c['kind'] == B.KIND_CONST
    exact['constant channels: var 0, mean exact'] = bool(np.all(v[const] == 0) and np.array_equal(m[const], y[0, const]))
    for decay, mm0, mv0, mm, mv, mean2, var2 in runs:
        exact['bn_stats_ema %g: the moments of bn_stats' % decay] = torch.equal(mean2, mean) and torch.equal(var2, var)
        exact['bn_stats_ema %g: moving mean' % decay] = B.ema_matches(host(mm), host(mm0), m, decay)
        exact['bn_stats_ema %g: moving var' % decay] = B.ema_matches(host(mv), host(mv0), v, decay)
        exact['bn_stats_ema %g: moving == batch stays' % decay] = bool(np.array_equal(host(mm)[::2], m[::2]) and np.array_equal(host(mv)[::2], v[::2]))
    report('bn_stats %dx%d %s' % (M, C, mode), ratios, exact)


@pytest.mark.parametrize('M,C,mode', STATS_RUNS)
def test_finalisation_conditioning(ops, M, C, mode):
    """bn_finalize, bn_leaky_fin and bn_leaky_pool_fin on host-built partial rows (exact sums, rounded once: c = 1) of y - shift with the shift at
    the mean and 1, 30, 300 std away, rows in {1, 5, 16, 256}.  The activations are checked against the oracle on the moments the kernel
    itself stored (read back): its apply arithmetic on its own; the moments have their own bound.  (The two backward *_fin consumers sum
    plain dgamma / dbeta rows, which have no shift; their backward decides on the sign of z, so they run on the lattice cases, where no
    z is near 0: test_lattice_fin_forms.)"""
    c = B.stats_case(M, C, mode)
    y, gamma, beta = c['y'], c['gamma'], c['beta']
    yd, g, b_ = upload(y, mode), dev(gamma), dev(beta)
    lda = ld_of(C, mode)
    pool = B.POOL_SHAPE_OF_M.get(M)
    runs = []
    for i, (placement, rows) in enumerate(B.fin_combos(M, C)):
        shift = B.placed_shift(y, placement)
        decay = B.EMA_DECAYS[i % 3]
        mm0, mv0 = B.placed_shift(y, '1std'), np.ones(C, f32)
        out = dict(placement=placement, rows=rows, shift=shift, decay=decay, mm0=mm0, mv0=mv0)
        part = dev(B.host_rows(y, shift, rows, poison=False))
        out['finalize'] = (nans(C), nans(C), dev(mm0), dev(mv0), part)
        ops.bn_finalize(part, dev(shift), M, C, out['finalize'][0], out['finalize'][1], out['finalize'][2], out['finalize'][3], decay)
        poisoned = dev(B.host_rows(y, shift, rows, poison=True))
        if fin_agrees(ops, rows, C, mode):
            mean, var, mm, mv, A = nans(C), nans(C), dev(mm0), dev(mv0), nans(M * lda, TD[mode])
            ops.bn_leaky_fin(yd, poisoned, rows, dev(shift), mean, var, mm, mv, decay, g, b_, A, M, C, lda, B.EPS, B.ALPHA)
            out['fin'] = (mean, var, mm, mv, A)
            if pool:
                Bn, H, W = pool
                MP = M // 4
                mean, var, mm, mv = nans(C), nans(C), dev(mm0), dev(mv0)
                P, idx = nans(MP * lda, TD[mode]), torch.full((MP * C,), 9, dtype=torch.uint8, device='cuda')
                ymax, afull = nans(MP * C, TD[mode]), nans(M * C, TD[mode])
                ops.bn_leaky_pool_fin(yd, poisoned, rows, dev(shift), mean, var, mm, mv, decay, g, b_, P, idx, Bn, H, W, C, lda, B.EPS, B.ALPHA,
                                      ymax=ymax, a_full=afull)
                out['pool_fin'] = (mean, var, mm, mv, P, idx, ymax, afull)
        else:
            with pytest.raises(HipKernelError, match=REFUSED):
                ops.bn_leaky_fin(yd, poisoned, rows, dev(shift), nans(C), nans(C), None, None, decay, g, b_, nans(M * lda, TD[mode]), M, C, lda, B.EPS, B.ALPHA)
        runs.append(out)
    torch.cuda.synchronize()
    const = c['kind'] == B.KIND_CONST
    leaky_beta = B.store32(np.maximum(beta, f32(B.ALPHA) * beta), mode).astype(np.float64)
    for out in runs:
        ratios, exact = {}, {}
        what = 'rows %s/%d %dx%d %s' % (out['placement'], out['rows'], M, C, mode)
        for key in ('finalize', 'fin', 'pool_fin'):
            if key not in out:
                continue
            mean, var, mm, mv = out[key][:4]
            m, v = moments(key + ' (c = 1)', mean, var, y, out['shift'], 1, ratios, exact)
            exact[key + ' moving mean'] = B.ema_matches(host(mm), out['mm0'], m, out['decay'])
            exact[key + ' moving var'] = B.ema_matches(host(mv), out['mv0'], v, out['decay'])
            if out['placement'] == 'mean':
                exact[key + ' constant channels: var 0, mean exact'] = bool(np.all(v[const] == 0) and np.array_equal(m[const], y[0, const]))
            if key == 'finalize':
                exact['finalize left its rows zero'] = float(out[key][4].abs().max()) == 0.0
                continue
            _, a_ref = B.fwd64(y, m, v, gamma, beta)
            if key == 'fin':
                a = unpad(out[key][4], M, C, lda, what + ' A')
                ratios['fin a'] = B.grad_ratio(a, a_ref, mode)
            else:
                Bn, H, W = pool
                MP = M // 4
                P, idx, ymax, afull = out[key][4:]
                w = B.windows(a_ref.reshape(Bn, H, W, C))
                ratios['pool_fin p'] = B.grad_ratio(unpad(P, MP, C, lda, what + ' P'), w.max(0).reshape(MP, C), mode)
                a = host(afull).astype(np.float64).reshape(M, C)
                ratios['pool_fin A_full'] = B.grad_ratio(a, a_ref, mode)
                arg = host(idx.float()).astype(np.int64).reshape(Bn, H // 2, W // 2, C)
                exact['pool_fin arg-max bytes in 0..3'] = bool(arg.max() <= 3)
                pick = B.take(B.windows(y.reshape(Bn, H, W, C)), np.minimum(arg, 3))
                exact['pool_fin ymax is y at the arg-max'] = bool(np.array_equal(host(ymax).reshape(pick.shape), pick))
                # the arg-max is the first maximum of the activations the kernel stored
                wst = B.windows(a.reshape(Bn, H, W, C))
                exact['pool_fin arg-max is the first maximum of A_full'] = bool(np.array_equal(wst.argmax(0), arg))
            if out['placement'] == 'mean':
                exact[key + ' constant channels give leaky(beta)'] = bool(np.all(a[:, const] == leaky_beta[const]))
        report(what, ratios, exact)


@pytest.mark.parametrize('shape,k,placement,mode', CONV_RUNS, ids=['%s-k%d-%s-%s' % ('x'.join(map(str, r[0])), r[1], r[2], r[3]) for r in CONV_RUNS])
def test_conv2d_bn_partial_rows_conditioning(ops, shape, k, placement, mode):
    """conv2d_bn as a producer of partial rows: output channels with means 0, 3, 30, 300 (std ~ 1), the shift at the chosen mean and 30 std
    away.  Reference: the float64 moments of the y the kernel STORED; c = M + 2 (one f32 chain over all samples: the rows may be shared
    between tiles in any order)."""
    Bn, H, W, Cin, Cout = shape
    M = Bn * H * W
    c = B.conv_case(shape, k)
    T = TD[mode]
    F = torch.zeros(Cout * k * k * Cin, dtype=T, device='cuda')
    ops.filter_prep(dev(c['w']), F, None, k, Cin, Cin, Cout, Cout, T)
    xd = dev(c['x'], T)
    ws = torch.full((1024 + 256 * 256 * 128,), 3.0, dtype=torch.float32, device='cuda')
    shift = (c['means'] + B.CONV_SHIFTS[placement]).astype(f32)
    y = torch.zeros(M * Cout, dtype=T, device='cuda')
    part = torch.zeros(2 * B.PART_ROWS * Cout, dtype=torch.float32, device='cuda')
    ops.conv2d_bn(xd, F, y, ws, Bn, H, W, Cin, Cin, Cout, Cout, k, dev(shift), part)
    rows_copy = part.clone()
    mean, var = nans(Cout), nans(Cout)
    ops.bn_finalize(part, dev(shift), M, Cout, mean, var, None, None, 0.999)
    torch.cuda.synchronize()
    yh = host(y).astype(np.float64).reshape(M, Cout)
    assert np.all(np.isfinite(yh))
    assert np.all(np.abs(yh.mean(0) - c['means']) < 1.0 + 0.01 * np.abs(c['means']))         # the chosen means arrived
    rows, s1, s2 = part_row_sums(ops, rows_copy, Cout)
    ratios, exact = {}, {}
    rm, rv = B.moment_ratios(*B.finalize64(s1, s2, shift, M), yh, shift, M + 2)
    ratios['rows (%d, c = %d) mean' % (rows, M + 2)], ratios['rows var'] = float(rm.max()), float(rv.max())
    moments('bn_finalize', mean, var, yh, shift, M + 2, ratios, exact)
    exact['bn_finalize left the rows zero'] = float(part.abs().max()) == 0.0
    report('conv2d_bn %s k%d %s %s' % (shape, k, placement, mode), ratios, exact)


# ---------------------------------------------------------------------------------------------------------------------
# B and C. channel counts and decision points, on the lattice cases
# ---------------------------------------------------------------------------------------------------------------------

def lattice_device(name, mode):
    c, ref = B.lattice_case(name, mode), B.lattice_reference(name, mode)
    par = tuple(dev(c[k]) for k in ('mean', 'var', 'gamma', 'beta'))
    return c, ref, upload(c['y'], mode), par


def part_sums(ws, rows, C):
    p = host(ws.view(torch.float32)[:2 * rows * C]).astype(np.float64).reshape(2, rows, C)
    return p[0].sum(0), p[1].sum(0)


@pytest.mark.parametrize('name,mode', B.LATTICE_RUNS)
def test_lattice_statistics(ops, name, mode):
    """bn_stats / bn_stats_ema at every channel count (the general reduction path with idle threads included)."""
    c = B.lattice_case(name, mode)
    M, C = c['M'], c['C']
    y = c['y'].reshape(M, C)
    yd = upload(y, mode)
    mean, var, mean2, var2 = nans(C), nans(C), nans(C), nans(C)
    mm0, mv0 = c['mean'] + f32(0.25), c['var']
    mm, mv = dev(mm0), dev(mv0)
    ops.bn_stats(yd, mean, var, workspace(C), M, C)
    ops.bn_stats_ema(yd, mean2, var2, mm, mv, 0.9, workspace(C), M, C)
    torch.cuda.synchronize()
    ratios, exact = {}, {}
    ct = B.chain_terms(M, C, B.VEC[mode])
    m, v = moments('bn_stats (c = %d)' % ct, mean, var, y, y[0], ct, ratios, exact)
    exact['bn_stats_ema: the moments of bn_stats'] = torch.equal(mean2, mean) and torch.equal(var2, var)
    exact['bn_stats_ema: moving averages'] = B.ema_matches(host(mm), mm0, m, 0.9) and B.ema_matches(host(mv), mv0, v, 0.9)
    report('statistics %s %s' % (name, mode), ratios, exact)


@pytest.mark.parametrize('name,mode', B.LATTICE_RUNS)
def test_lattice_two_launch_forms(ops, name, mode):
    """bn_leaky, bn_leaky_bwd_reduce, bn_leaky_bwd_reduce_part and bn_leaky_bwd_apply; mean, var, dgamma and dbeta are the case's inputs."""
    c, ref, yd, par = lattice_device(name, mode)
    M, C, T = c['M'], c['C'], TD[mode]
    ld = ld_of(C, mode)
    A = nans(M * ld, T)
    ops.bn_leaky(yd, *par, A, M, C, ld, B.EPS, B.ALPHA)
    dad = upload(c['da'].reshape(M, C), mode, ld)
    dg, db = nans(C), nans(C)
    ops.bn_leaky_bwd_reduce(dad, ld, yd, *par, dg, db, workspace(C), M, C, B.EPS, B.ALPHA)
    ws = workspace(C)
    rows = ops.bn_leaky_bwd_reduce_part(dad, ld, yd, *par, ws, 1024, M, C, B.EPS, B.ALPHA)
    dY = nans(M * C, T)
    ops.bn_leaky_bwd_apply(dad, ld, yd, *par, dev(c['dgamma_in']), dev(c['dbeta_in']), dY, M, C, B.EPS, B.ALPHA)
    torch.cuda.synchronize()
    ct = B.chain_terms(M, C, B.VEC[mode])
    assert rows == B.colsum_grid(M, C, B.VEC[mode])
    a = unpad(A, M, C, ld, 'A')
    z = ref['z'].reshape(M, C)
    dy = host(dY).astype(np.float64)
    s_gx, s_g = part_sums(ws, rows, C)
    ratios = {'a': B.grad_ratio(a, ref['a'].reshape(M, C), mode), 'dy': B.grad_ratio(dy.reshape(ref['dy'].shape), ref['dy'], mode),
              'dgamma (c = %d)' % ct: float(B.reduced_ratio(host(dg), ref['gx'], ct).max()), 'dbeta': float(B.reduced_ratio(host(db), ref['g'], ct).max()),
              'dgamma (rows)': float(B.reduced_ratio(s_gx, ref['gx'], ct).max()), 'dbeta (rows)': float(B.reduced_ratio(s_g, ref['g'], ct).max())}
    exact = {'a is 0 where z is exactly 0': bool(np.all(a[z == 0] == 0)), 'dy written everywhere': not np.isnan(dy).any()}
    report('two-launch %s %s' % (name, mode), ratios, exact)


POOLED_RUNS = [(n, m) for n, m in B.LATTICE_RUNS if B.LATTICE[n][1] % 2 == 0 and B.LATTICE[n][2] % 2 == 0]


@pytest.mark.parametrize('name,mode', POOLED_RUNS)
def test_lattice_pooled_forms(ops, name, mode):
    """bn_leaky_pool, bn_leaky_pool_bwd_reduce, bn_leaky_pool_bwd_reduce_part and bn_leaky_pool_bwd_apply.  The arg-max bytes equal the reference's
    (first maximum of the activations rounded to the storage type); the backward kernels read the REFERENCE's arg-max bytes."""
    c, ref, yd, par = lattice_device(name, mode)
    Bn, H, W, C, M, T = c['B'], c['H'], c['W'], c['C'], c['M'], TD[mode]
    MP = M // 4
    ld = ld_of(C, mode)
    P, idx = nans(MP * ld, T), torch.full((MP * C,), 9, dtype=torch.uint8, device='cuda')
    ops.bn_leaky_pool(yd, *par, P, idx, Bn, H, W, C, ld, B.EPS, B.ALPHA)
    arg_d = torch.from_numpy(np.ascontiguousarray(ref['arg'])).to('cuda')
    dpd = upload(c['dp'].reshape(MP, C), mode, ld)
    dg, db = nans(C), nans(C)
    ops.bn_leaky_pool_bwd_reduce(dpd, ld, arg_d, yd, *par, dg, db, workspace(C), Bn, H, W, C, B.EPS, B.ALPHA)
    ws = workspace(C)
    rows = ops.bn_leaky_pool_bwd_reduce_part(dpd, ld, arg_d, yd, *par, ws, 1024, Bn, H, W, C, B.EPS, B.ALPHA)
    dY = nans(M * C, T)
    ops.bn_leaky_pool_bwd_apply(dpd, ld, arg_d, yd, *par, dev(c['dgamma_in']), dev(c['dbeta_in']), dY, Bn, H, W, C, B.EPS, B.ALPHA)
    torch.cuda.synchronize()
    ct = B.chain_terms(MP, C, B.VEC[mode])
    assert rows == B.colsum_grid(MP, C, B.VEC[mode])
    p = unpad(P, MP, C, ld, 'P').reshape(ref['p'].shape)
    s_gx, s_g = part_sums(ws, rows, C)
    ratios = {'p': B.grad_ratio(p, ref['p'], mode), 'dy': B.grad_ratio(host(dY).astype(np.float64).reshape(ref['pdy'].shape), ref['pdy'], mode),
              'dgamma (c = %d)' % ct: float(B.reduced_ratio(host(dg), ref['pgx'], ct).max()), 'dbeta': float(B.reduced_ratio(host(db), ref['pg'], ct).max()),
              'dgamma (rows)': float(B.reduced_ratio(s_gx, ref['pgx'], ct).max()), 'dbeta (rows)': float(B.reduced_ratio(s_g, ref['pg'], ct).max())}
    exact = {'arg-max bytes': bool(np.array_equal(idx.cpu().numpy().reshape(ref['arg'].shape), ref['arg'])),
             'p is 0 where the maximum is exactly 0': bool(np.all(p[ref['p'] == 0] == 0)),
             'p is exactly 1 in the collision channels': bool(np.all(p[..., c['collide']] == 1.0))}
    report('pooled %s %s' % (name, mode), ratios, exact)


@pytest.mark.parametrize('name,mode', B.LATTICE_RUNS)
def test_lattice_fin_forms(ops, name, mode):
    """bn_leaky_fin, bn_leaky_pool_fin, bn_leaky_bwd_apply_fin and bn_leaky_pool_bwd_apply_fin where bn_fin_supported says yes; where it says no,
    all four are refused with the library's argument error.  The forward rows are ones whose finalisation is exact (bn_cases.exact_rows), so
    the kernels normalise with exactly the case's mean and var and every decision of the lattice holds; the backward rows are the exact
    sums of the reference's terms, rounded once (c = 1), and dy is checked against the oracle on the dgamma / dbeta the kernel stored."""
    c, ref, yd, par = lattice_device(name, mode)
    Bn, H, W, C, M, T = c['B'], c['H'], c['W'], c['C'], c['M'], TD[mode]
    mean_in, var_in, g, b_ = par
    rows = B.FIN_ROWS[list(B.LATTICE).index(name) % 4]
    ld = ld_of(C, mode)
    MP = M // 4
    part = dev(B.exact_rows(c['fin_s2'], rows))
    bpart = dev(B.host_term_rows(ref['gx'], ref['g'], rows, rows, False))
    dad = upload(c['da'].reshape(M, C), mode, ld)
    A, dY, pdY = nans(M * ld, T), nans(M * C, T), nans(M * C, T)
    mean, var, mean2, var2, dg, db, pdg, pdb = (nans(C) for _ in range(8))
    mm0, mv0 = c['mean'] - f32(0.5), c['var'] * f32(2)
    mm, mv = dev(mm0), dev(mv0)
    P, idx = nans(MP * ld, T), torch.full((MP * C,), 9, dtype=torch.uint8, device='cuda')
    ymax, afull = nans(MP * C, T), nans(M * C, T)
    if c['pooled']:
        arg_d = torch.from_numpy(np.ascontiguousarray(ref['arg'])).to('cuda')
        dpd = upload(c['dp'].reshape(MP, C), mode, ld)
        pbpart = dev(B.host_term_rows(ref['pgx'], ref['pg'], rows, rows, False))
    calls = [lambda: ops.bn_leaky_fin(yd, part, rows, mean_in, mean, var, mm, mv, 0.9, g, b_, A, M, C, ld, B.EPS, B.ALPHA),
             lambda: ops.bn_leaky_bwd_apply_fin(dad, ld, yd, *par, bpart, rows, rows * C, dg, db, dY, M, C, B.EPS, B.ALPHA)]
    if c['pooled']:
        calls += [lambda: ops.bn_leaky_pool_fin(yd, part, rows, mean_in, mean2, var2, None, None, 0.9, g, b_, P, idx, Bn, H, W, C, ld, B.EPS, B.ALPHA,
                                                ymax=ymax, a_full=afull),
                  lambda: ops.bn_leaky_pool_bwd_apply_fin(dpd, ld, arg_d, yd, *par, pbpart, rows, rows * C, pdg, pdb, pdY, Bn, H, W, C, B.EPS, B.ALPHA)]
    if not fin_agrees(ops, rows, C, mode):
        for call in calls:
            with pytest.raises(HipKernelError, match=REFUSED):
                call()
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t.float()).all()) for t in (A, dY, pdY, mean, var, dg, db, P))        # nothing was launched
        return
    for call in calls:
        call()
    torch.cuda.synchronize()
    a = unpad(A, M, C, ld, 'A')
    z = ref['z'].reshape(M, C)
    dgh, dbh = host(dg), host(db)
    dy_ref = B.bwd_apply64(c['y'], c['da'], c['mean'], c['var'], c['gamma'], c['beta'], dgh, dbh, M)
    ratios = {'a': B.grad_ratio(a, ref['a'].reshape(M, C), mode), 'dgamma (c = 1)': float(B.reduced_ratio(dgh, ref['gx'], 1).max()),
              'dbeta': float(B.reduced_ratio(dbh, ref['g'], 1).max()), 'dy': B.grad_ratio(host(dY).astype(np.float64).reshape(dy_ref.shape), dy_ref, mode)}
    exact = {'mean and var are exactly the rows\' own': torch.equal(mean, mean_in) and torch.equal(var, var_in),
             'moving averages': B.ema_matches(host(mm), mm0, c['mean'], 0.9) and B.ema_matches(host(mv), mv0, c['var'], 0.9),
             'a is 0 where z is exactly 0': bool(np.all(a[z == 0] == 0))}
    if c['pooled']:
        p = unpad(P, MP, C, ld, 'P').reshape(ref['p'].shape)
        pdgh, pdbh = host(pdg), host(pdb)
        pdy_ref = B.bwd_apply64(c['y'], B.route(c['dp'].astype(np.float64), ref['arg']), c['mean'], c['var'], c['gamma'], c['beta'], pdgh, pdbh, M)
        ratios.update({'p': B.grad_ratio(p, ref['p'], mode), 'A_full': B.grad_ratio(host(afull).astype(np.float64).reshape(ref['a'].shape), ref['a'], mode),
                       'pooled dgamma (c = 1)': float(B.reduced_ratio(pdgh, ref['pgx'], 1).max()), 'pooled dbeta': float(B.reduced_ratio(pdbh, ref['pg'], 1).max()),
                       'pooled dy': B.grad_ratio(host(pdY).astype(np.float64).reshape(pdy_ref.shape), pdy_ref, mode)})
        exact.update({'pooled mean and var': torch.equal(mean2, mean_in) and torch.equal(var2, var_in),
                      'arg-max bytes': bool(np.array_equal(idx.cpu().numpy().reshape(ref['arg'].shape), ref['arg'])),
                      'ymax is y at the arg-max, bit for bit': bool(np.array_equal(host(ymax).astype(np.float64).reshape(ref['ymax'].shape), ref['ymax'])),
                      'p is 0 where the maximum is exactly 0': bool(np.all(p[ref['p'] == 0] == 0)),
                      'p is exactly 1 in the collision channels': bool(np.all(p[..., c['collide']] == 1.0))})
    report('fin (rows %d) %s %s' % (rows, name, mode), ratios, exact)


# ---------------------------------------------------------------------------------------------------------------------
# D. moving averages
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('decay', B.EMA_DECAYS)
@pytest.mark.parametrize('C', [8, 300, 1024])
def test_bn_ema_bit_exact(ops, C, decay):
    """bn_ema: moving -= (1 - decay) * (moving - batch), bit-equal to the f32 restatement; moving values far from and EQUAL to the batch's."""
    rng = np.random.RandomState(C)
    mean, var = (rng.randn(C) * 3).astype(f32), (rng.rand(C) * 4).astype(f32)
    mm0 = np.where(np.arange(C) % 2 == 0, mean, mean + f32(100) * rng.randn(C).astype(f32)).astype(f32)
    mv0 = np.where(np.arange(C) % 2 == 0, var, rng.rand(C).astype(f32) * f32(1e3)).astype(f32)
    mm, mv = dev(mm0), dev(mv0)
    ops.bn_ema(mm, mv, dev(mean), dev(var), C, decay)
    torch.cuda.synchronize()
    assert B.ema_matches(host(mm), mm0, mean, decay) and B.ema_matches(host(mv), mv0, var, decay)
    assert np.array_equal(host(mm)[::2], mean[::2]) and np.array_equal(host(mv)[::2], var[::2])
