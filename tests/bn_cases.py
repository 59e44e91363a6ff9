"""Inputs, float64 references and error bounds for the batch-norm family (csrc/bn.hip, csrc/bn_stats.hip, csrc/bn_leaky.h, csrc/colsum.h):
statistics, BN + leaky ReLU (+ 2x2 max pool) forward and backward, the consumers that finalise partial rows themselves (*_fin), and the
moving averages.  NumPy and oracle/yolo2_ref.py only: tests/test_bn_cases_cpu.py checks the cases, the restated launch geometry and the
bounds on a machine without a GPU, tests/test_bn_gpu.py launches the kernels on them.

The reference is the oracle in float64 on exactly the values a kernel reads (tensors rounded to bf16 first in bf16 mode, f32 per-channel
vectors widened unchanged, eps and alpha as the f32 numbers the ABI passes).  A kernel that takes mean, var, dgamma or dbeta as INPUTS gets
values chosen by the case: it is tested on its own arithmetic, not on its predecessor's error.

Four groups of cases:
  A  statistics conditioning (STATS_SHAPES): mean / std ratios 0 .. 3000 side by side in one tensor, constant channels, an outlier, a
     channel at mean 1000 / std 4; the shift of the single-pass moments at the mean, 1, 30 and 300 std away;
  B  channel counts (CHANNELS x LATTICE_SHAPES): every C the entry points admit around the threads-per-row values that do not divide 256;
  C  decision points (DECISION_CASES): exact zeros of z, negative gamma, planted pool windows;
  D  moving averages (EMA_DECAYS).
B and C share one generator, `lattice_case`: per channel y = mu_c + k * delta_c with integer k in [-16, 16] and mean = mu_c given as an
input, so every z is either exactly 0 or far from 0 and two activations of a pool window are either bit-equal or far apart (`conditions`
measures this for EVERY element and EVERY window; a seed or lattice that violated MARGIN would be replaced, never the margin).

Bounds (derived, not fitted).  u = 2^-24, d = y - s in float64 for the shift s, E2 = mean(d^2), E1 = mean|d|, dm = mean(d):
  |mean - mean_ref| <= 1e-6 |mean_ref| + c u E1 + u |mean_ref|                      (the last term is the f32 store)
  |var  - var_ref | <= 1e-5 var_ref + c u (E2 + 2 |dm| E1)
  |dgamma - ref|, |dbeta - ref| <= 1e-5 |ref| + c u sum|term|                        (terms g * xhat and g in float64)
c is the largest number of terms any single f32 accumulator sums before the f64 finalisation, plus 2 (the subtraction and the product
that form a term):
  bn_stats, bn_stats_ema, bn_leaky_bwd_reduce(_part), bn_leaky_pool_bwd_reduce(_part):  c = rows per thread + rpp + 2, read off the
      restated RowMap and colsum_grid (`chain_terms`: a thread's own rows, then at most rpp row slots meet in one accumulator -- the
      general path sums them serially, the lane-group paths as a tree of 64 / tpr lanes plus four waves, which is fewer);
  host-built partial rows (bn_finalize and the *_fin consumers):  c = 1 -- each row is an exact float64 sum of float64 terms, rounded
      to f32 once;
  conv2d_bn as a producer:  c = M + 2 -- its rows may be shared between tiles through f32 atomics in any order, and one f32 chain over
      all M samples is the worst any order can do.
The variance bound carries the term 2 |dm| E1 that a bound of the form c u E2 alone leaves out: var = E2 - dm^2, so an error of
c u E1 in dm moves the variance by 2 |dm| c u E1, which equals 2 c u E2 once the shift is far from the mean.  A single correctly rounded
row (rows = 1, shift 300 std away) already exceeds c u E2 in some channels (tests/test_bn_cases_cpu.py shows it), so the term is part of
the derivation and not room for the kernel.  Elementwise outputs (a, pooled p, ymax, A_full, dy): head_cases.f32_ratio in f32, bf16_ratio
in bf16.  Arg-max bytes and moving averages: exact.

How far may the shift be from the batch mean?  With the shift k std away E2 = (1 + k^2) var and |dm| E1 ~ k^2 var, so the variance
bound is c u (1 + 3 k^2) relative to the variance; it reaches the project's 1e-4 at k = sqrt((1e-4 / (c u) - 1) / 3):

      c      kernel (example)                                             k (std) at which the bound is 1e-4 var
      1      host-built rows                                              23.6
     10      bn_stats C = 1024 bf16, M = 2704 (6 rows + rpp 2 + 2)        7.5
     27      bn_stats C = 96 bf16, M = 1352 (4 rows + rpp 21 + 2)         4.5
    134      bn_stats C = 8 f32, M = 2704 (4 rows + rpp 128 + 2)          2.0
    340      conv2d_bn, M = 338                                           1.1
    678      conv2d_bn, M = 676                                           0.70
(`shift_distance(c)`).  bn_stats shifts by the channel's first sample, which is ~1 std from the mean; the training engine shifts by the
MOVING mean, which follows the batch mean with decay 0.999 -- early in training, or after a jump of the learning rate, it can be many
std away, and the numbers above say how many before the f32 tolerance of the variance is gone."""
import fractions
import functools

import numpy as np

from oracle import yolo2_ref as R
from head_cases import MODES, MARGIN, F32_RTOL, f32_ratio, bf16_ratio, grad_ratio, stored, bf16_truncate, inputs64      # noqa: F401

U = 2.0 ** -24
EPS = float(np.float32(1e-5))       # what the ABI's float arguments hold
ALPHA = float(np.float32(0.1))
VEC = {'f32': 4, 'bf16': 8}
PART_ROWS = 256                     # include/yolo2_hip.h YOLO2_BN_PART_ROWS
BF16_ULP = 2.0 ** -7                # one bf16 ulp of x is at most 2^-7 |x|
EMA_DECAYS = (0.999, 0.9, 0.0)


# ------------------------------------------------------------------------------------------------------------------
# launch geometry, restated from csrc/colsum.h (RowMap, colsum_grid) and csrc/bn.hip (rowmap_grid)
# ------------------------------------------------------------------------------------------------------------------

class RowMap(object):
    """csrc/colsum.h RowMap for the 256 threads of a workgroup: a fixed channel group per thread, rows strided."""

    def __init__(self, C, vec):
        t = np.arange(256)
        self.tpr = C // vec
        self.rpp = max(256 // self.tpr, 1)
        self.cg = t % self.tpr
        self.rs = t // self.tpr
        self.active = (self.rs < self.rpp) & (t < self.tpr * self.rpp)


def colsum_grid(M, C, vec):
    """csrc/colsum.h colsum_grid."""
    tpr = C // vec
    rpp = max(256 // tpr, 1)
    return int(max(min((M + rpp * 4 - 1) // (rpp * 4), 256), 1))


def rowmap_grid(M, C, vec, rows_per_thread):
    """csrc/bn.hip rowmap_grid."""
    tpr = C // vec
    rpp = max(256 // tpr, 1)
    return int(max(min((M + rpp * rows_per_thread - 1) // (rpp * rows_per_thread), 4096), 1))


# kernel -> (grid rule, has the four-way unrolled loop in front of its single-row loop); `rows` is M, or the pooled pixel count
KERNELS = {
    'bn_stats':                 (lambda rows, C, vec: colsum_grid(rows, C, vec), True),        # colsum_kernel<T, 2>
    'bn_leaky_bwd_reduce':      (lambda rows, C, vec: colsum_grid(rows, C, vec), True),        # bn_bwd_reduce_kernel (+ _part: same grid at these sizes)
    'bn_leaky':                 (lambda rows, C, vec: rowmap_grid(rows, C, vec, 4), False),
    'bn_leaky_bwd_apply':       (lambda rows, C, vec: rowmap_grid(rows, C, vec, 4), False),
    'bn_leaky_pool':            (lambda rows, C, vec: rowmap_grid(rows, C, vec, 2), False),    # rows = pooled pixels
    'bn_leaky_pool_bwd_apply':  (lambda rows, C, vec: rowmap_grid(rows, C, vec, 2), False),
    'bn_leaky_pool_bwd_reduce': (lambda rows, C, vec: colsum_grid(rows, C, vec), False),
}


def thread_slots(rows, C, vec, grid):
    """(first row, channel group) of every ACTIVE thread of every workgroup, and the row step of the loops."""
    rm = RowMap(C, vec)
    act = np.flatnonzero(rm.active)
    first = (np.arange(grid)[:, None] * rm.rpp + rm.rs[act][None, :]).reshape(-1)
    cg = np.broadcast_to(rm.cg[act][None, :], (grid, len(act))).reshape(-1)
    return first, cg, grid * rm.rpp


def coverage(rows, C, vec, grid):
    """visits [rows, tpr]: how many active threads of the launch touch each (row, channel group); plus the largest channel and row touched."""
    first, cg, step = thread_slots(rows, C, vec, grid)
    visits = np.zeros((rows, C // vec), np.int64)
    top_row = -1
    r = first.copy()
    while True:
        ok = r < rows                   # the loops' own condition
        if not ok.any():
            break
        np.add.at(visits, (r[ok], cg[ok]), 1)
        top_row = max(top_row, int(r[ok].max()))
        r = r + step
    return visits, int(cg.max()) * vec + vec, top_row


def rows_per_thread(rows, C, vec, grid):
    first, _, step = thread_slots(rows, C, vec, grid)
    return np.where(first < rows, (rows - first + step - 1) // step, 0)


def loop_profile(rows, C, vec, grid):
    """Which parts of `for (; r + 3 * step < M; r += 4 * step)` + `for (; r < M; r += step)` run: (unrolled, tail, ragged).  ragged: the
    threads of one launch do not all take the same number of rows (the last step is partly beyond the end)."""
    n = rows_per_thread(rows, C, vec, grid)
    return bool((n // 4 > 0).any()), bool((n % 4 > 0).any()), bool(n.min() != n.max())


def chain_terms(rows, C, vec, grid=None):
    """c of the bounds for a column reduction: a thread's own rows, then the rpp row slots of a workgroup, plus 2."""
    grid = colsum_grid(rows, C, vec) if grid is None else grid
    return int(rows_per_thread(rows, C, vec, grid).max()) + max(256 // (C // vec), 1) + 2


def fin_supported(rows, C, vec):
    """csrc/bn.hip fin_shape_ok (what yolo2_bn_fin_supported answers)."""
    if rows < 1 or C < vec or C % vec:
        return False
    tpr = C // vec
    if tpr & (tpr - 1):
        return False
    return rows * min(tpr, 16) * vec * 8 <= (128 << 10)


def shift_distance(c, tol=1e-4):
    """Shift distance in std at which the variance bound c u (1 + 3 k^2) var reaches tol * var (None: it is never below tol)."""
    x = (tol / (c * U) - 1) / 3
    return float(np.sqrt(x)) if x > 0 else None


# ------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------

def _ratio(err, bound):
    """err / bound per element; 0 where both are 0 (an exact result that is exact), inf where only the bound is."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(err == 0, 0.0, err / bound)


def moment_refs(y64, shift64):
    d = y64 - shift64
    mean = y64.mean(0)
    return dict(mean=mean, var=((y64 - mean) ** 2).mean(0), E2=(d * d).mean(0), E1=np.abs(d).mean(0), dm=d.mean(0))


def moment_ratios(mean, var, y64, shift64, c, issue_form=False):
    """Per channel |err| / bound of a batch mean and a biased batch variance computed with the shift `shift64` (see the module docstring).
    issue_form: the variance bound without the mean plane's contribution, c u E2 alone."""
    m = moment_refs(np.asarray(y64, np.float64), np.asarray(shift64, np.float64))
    mean, var = np.asarray(mean, np.float64), np.asarray(var, np.float64)
    bm = 1e-6 * np.abs(m['mean']) + c * U * m['E1'] + U * np.abs(m['mean'])
    bv = 1e-5 * m['var'] + c * U * (m['E2'] + (0 if issue_form else 2 * np.abs(m['dm']) * m['E1']))
    return _ratio(np.abs(mean - m['mean']), bm), _ratio(np.abs(var - m['var']), bv)


def reduced_ratio(got, terms64, c):
    """Per channel |err| / (1e-5 |ref| + c u sum|term|) of a column sum of `terms64` [rows, C]."""
    ref = terms64.sum(0)
    return _ratio(np.abs(np.asarray(got, np.float64) - ref), 1e-5 * np.abs(ref) + c * U * np.abs(terms64).sum(0))


# ------------------------------------------------------------------------------------------------------------------
# float64 references
# ------------------------------------------------------------------------------------------------------------------

def fwd64(y, mean, var, gamma, beta):
    """(z, a) of BN + leaky ReLU."""
    z = R.bn_apply(np.asarray(y, np.float64), *(np.asarray(v, np.float64) for v in (mean, var, gamma, beta)), eps=EPS)
    return z, R.leaky_relu(z, ALPHA)


def bwd_terms64(y, da, mean, var, gamma, beta):
    """(g, g * xhat): the summands of dbeta and dgamma."""
    y, da, mean, var = (np.asarray(v, np.float64) for v in (y, da, mean, var))
    z, _ = fwd64(y, mean, var, gamma, beta)
    g = R.leaky_relu_grad(z, da, ALPHA)
    return g, g * ((y - mean) / np.sqrt(var + EPS))


def bwd_apply64(y, da, mean, var, gamma, beta, dgamma, dbeta, count):
    """oracle bn_train_bwd's dx with dgamma / dbeta as INPUTS: (gamma * inv) * (g - dbeta / n - xhat * dgamma / n)."""
    y, da, mean, var, gamma, dgamma, dbeta = (np.asarray(v, np.float64) for v in (y, da, mean, var, gamma, dgamma, dbeta))
    g, _ = bwd_terms64(y, da, mean, var, gamma, beta)
    inv = 1.0 / np.sqrt(var + EPS)
    return (gamma * inv) * (g - dbeta / count - (y - mean) * inv * (dgamma / count))


def windows(x):
    """[B, H, W, C] -> [4, B, H/2, W/2, C], positions in scan order (0,0), (0,1), (1,0), (1,1)."""
    return np.stack([x[:, i::2, j::2, :] for i in range(2) for j in range(2)], 0)


def unwindows(w):
    k, B, OH, OW, C = w.shape
    x = np.zeros((B, OH * 2, OW * 2, C), w.dtype)
    for p in range(4):
        x[:, p // 2::2, p % 2::2, :] = w[p]
    return x


def take(w, arg):
    return np.take_along_axis(w, arg[None].astype(np.int64), 0)[0]


def route(dp, arg):
    """The pooled gradient at the arg-max position of every window, 0 elsewhere: [B, H, W, C]."""
    return unwindows(np.where(np.arange(4).reshape(4, 1, 1, 1, 1) == arg[None], dp[None], 0.0))


# ------------------------------------------------------------------------------------------------------------------
# f32 restatement of the kernels' arithmetic (expression order of csrc/bn_leaky.h), with switches for the mistakes a kernel could make
# ------------------------------------------------------------------------------------------------------------------
MUTATIONS = ('unshifted', 'shift_sum_plane_only', 'unbiased', 'eps_outside_sqrt', 'z_gt_0', 'sign_of_y_minus_mean', 'truncating_store',
             'last_max', 'argmax_unrounded', 'pooled_count', 'decay_swapped', 'no_clamp')
f32 = np.float32


def inv_std32(var, mut=None):
    var = np.asarray(var, f32)
    if mut == 'eps_outside_sqrt':
        return f32(1) / (np.sqrt(var) + f32(EPS))
    return f32(1) / np.sqrt(var + f32(EPS))


def fwd32(y, mean, var, gamma, beta, mut=None):
    """bn_leaky.h bn_leaky: z = (y - mu) * sc + bt with sc = inv_std * gamma; max(z, alpha z).  f32 -> (z, a)."""
    sc = inv_std32(var, mut) * np.asarray(gamma, f32)
    z = (np.asarray(y, f32) - np.asarray(mean, f32)) * sc + np.asarray(beta, f32)
    return z, np.maximum(z, f32(ALPHA) * z)


def store32(x, mode, mut=None):
    """The kernel's store of an f32 value: as it is, or rounded to bf16 (round-to-nearest-even)."""
    x = np.asarray(x, f32)
    if mode == 'f32':
        return x
    return bf16_truncate(x) if mut == 'truncating_store' else R.bf16_round(x)


def bwd_terms32(y, da, mean, var, gamma, beta, mut=None):
    """bn_leaky.h bn_leaky_bwd -> (g, xh)."""
    y, da, mean, gamma, beta = (np.asarray(v, f32) for v in (y, da, mean, gamma, beta))
    inv = inv_std32(var, mut)
    xh = (y - mean) * inv
    z = (y - mean) * (inv * gamma) + beta
    if mut == 'z_gt_0':
        pos = z > 0
    elif mut == 'sign_of_y_minus_mean':
        pos = (y - mean) >= 0
    else:
        pos = z >= 0
    return np.where(pos, da, f32(ALPHA) * da), xh


def bwd_apply32(y, da, mean, var, gamma, beta, dgamma, dbeta, count, mut=None):
    """bn_leaky.h bn_bwd_apply with dgm = dgamma * (1 / count), dbm = dbeta * (1 / count)."""
    g, xh = bwd_terms32(y, da, mean, var, gamma, beta, mut)
    inv_m = f32(1) / f32(count)
    return (np.asarray(gamma, f32) * inv_std32(var, mut)) * (g - np.asarray(dbeta, f32) * inv_m - xh * (np.asarray(dgamma, f32) * inv_m))


def pool32(a_rounded, a_f32, mode, mut=None):
    """bn_leaky.h pool_first_max on the activations rounded to T -> (arg [B, OH, OW, C] uint8, maximum)."""
    w = windows(a_f32 if mut == 'argmax_unrounded' else a_rounded)
    arg = (3 - w[::-1].argmax(0)) if mut == 'last_max' else w.argmax(0)
    return arg.astype(np.uint8), take(windows(a_rounded), arg)


def chain_sums32(terms, C, vec, grid):
    """Partial rows [grid, C] f32 of a column reduction over `terms` [rows, C] f32 with the restated geometry: every thread adds its rows in
    order in f32, then the rpp row slots of a workgroup are added in order in f32 (block_colsum_store's general path)."""
    terms = np.asarray(terms, f32)
    rows = terms.shape[0]
    rpp = max(256 // (C // vec), 1)
    step = grid * rpp
    n = (rows + step - 1) // step
    padded = np.zeros((n * step, C), f32)
    padded[:rows] = terms
    padded = padded.reshape(n, step, C)
    acc = np.zeros((step, C), f32)
    for i in range(n):
        acc = acc + padded[i]
    acc = acc.reshape(grid, rpp, C)
    out = np.zeros((grid, C), f32)
    for r in range(rpp):
        out = out + acc[:, r]
    return out


def finalize64(s0, s1, shift, count, mut=None):
    """reduce_finalize_kernel<0> / bn_finalize_kernel<0> / the *_fin prologue: f64 sums of the two planes -> (mean, var) in f32."""
    s0, s1 = np.asarray(s0, np.float64), np.asarray(s1, np.float64)
    dm = s0 / count
    var = s1 / count - dm * dm
    if mut == 'unbiased':
        var = var * count / max(count - 1, 1)
    if mut != 'no_clamp':
        var = np.where(var > 0, var, 0.0)
    return (np.asarray(shift, np.float64) + dm).astype(f32), var.astype(f32)


def stats32(y, shift, C, vec, grid, mut=None):
    """colsum_kernel<T, 2> + reduce_finalize_kernel<0>: shifted single-pass moments, f32 chains, f64 finalisation."""
    y = np.asarray(y, f32)
    sh = np.zeros(C, f32) if mut == 'unshifted' else np.asarray(shift, f32)
    x = y - sh
    sq = y * y if mut == 'shift_sum_plane_only' else x * x
    p0, p1 = chain_sums32(x, C, vec, grid), chain_sums32(sq, C, vec, grid)
    return finalize64(p0.astype(np.float64).sum(0), p1.astype(np.float64).sum(0), sh, y.shape[0], mut)


def host_rows(y, shift, rows, plane_rows=PART_ROWS, poison=True):
    """[2][plane_rows][C] f32 partial rows of sum(y - shift), sum((y - shift)^2): sample r goes to row r % rows; every row is the exact
    float64 sum of float64 terms, rounded to f32 once.  Rows beyond `rows` hold NaN when `poison` (a *_fin consumer must not read them)."""
    d = np.asarray(y, np.float64) - np.asarray(shift, np.float64)
    return host_term_rows(d, d * d, rows, plane_rows, poison)


def host_term_rows(t0, t1, rows, plane_rows, poison):
    part = np.full((2, plane_rows, t0.shape[1]), np.nan if poison else 0.0, f32)
    for k, t in enumerate((t0, t1)):
        for r in range(rows):
            part[k, r] = t[r::rows].sum(0) if r < t.shape[0] else 0.0
    return part


def exact_rows(s2, rows, plane_rows=PART_ROWS):
    """[2][plane_rows][C] partial rows whose finalisation is exact: plane 0 sums to 0 (+3 in row 0, -3 in the last row when there are two),
    plane 1 holds s2 in the LAST of the `rows` rows; NaN beyond `rows`."""
    part = np.full((2, plane_rows, len(s2)), np.nan, f32)
    part[:, :rows] = 0
    if rows > 1:
        part[0, 0], part[0, rows - 1] = 3.0, -3.0
    part[1, rows - 1] = s2
    return part


def rows_moments(part, rows, shift, count, mut=None):
    p = part[:, :rows].astype(np.float64)
    return finalize64(p[0].sum(0), p[1].sum(0), shift, count, mut)


def _round_f32(q):
    """A rational number -> the nearest f32, ties to even."""
    x = f32(float(q))
    best = None
    for cand in (np.nextafter(x, f32(-np.inf)), x, np.nextafter(x, f32(np.inf))):
        err = abs(fractions.Fraction(float(cand)) - q)
        even = (int(np.asarray(cand, f32).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, cand)
    return best[1]


def ema32(moving, batch, decay, mut=None):
    """bn_leaky.h bn_ema: m - (m - x) * omd with omd = (float)(1.0 - decay), in f32.  bn_stats.hip and bn.hip are built with floating-point
    contraction allowed, so the compiler may or may not fuse the product into the subtraction: -> (separately rounded, fused), and a
    kernel's result must equal one of the two in every element."""
    m, x = np.asarray(moving, f32), np.asarray(batch, f32)
    omd = f32(decay) if mut == 'decay_swapped' else f32(1.0 - decay)
    t = m - x
    plain = m - t * omd
    fused = np.array([_round_f32(fractions.Fraction(float(a)) - fractions.Fraction(float(b)) * fractions.Fraction(float(omd)))
                      for a, b in zip(m.reshape(-1), t.reshape(-1))], f32).reshape(m.shape)
    return plain, fused


def ema_matches(got, moving, batch, decay, mut=None):
    plain, fused = ema32(moving, batch, decay, mut)
    got = np.asarray(got, f32)
    return bool(np.all((got == plain) | (got == fused)))


# ------------------------------------------------------------------------------------------------------------------
# A. statistics conditioning
# ------------------------------------------------------------------------------------------------------------------
STATS_M = (4, 105, 676, 2704)
STATS_C = (8, 32, 1024)
STATS_SHAPES = [(M, C) for M in STATS_M for C in STATS_C]
POOL_SHAPE_OF_M = {4: (1, 2, 2), 676: (1, 26, 26), 2704: (4, 26, 26)}          # 105 is odd: no pooled form
RATIOS = (0, 3, 30, 300, 3000)                                                  # |mean| / std of channel kinds 0 .. 4
KIND_CONST, KIND_OUTLIER, KIND_BINADE = 5, 6, 7
CONSTANTS = (2.5, -7.0, 0.375, 96.0)                                            # exact in bf16
STD = 1.5
PLACEMENTS = {'mean': 0.0, '1std': 1.0, '30std': 30.0, '300std': 300.0}
FIN_ROWS = (1, 5, 16, 256)


@functools.lru_cache(maxsize=None)
def stats_case(M, C, mode):
    """dict: y [M, C] f32 (rounded to bf16 in bf16 mode), kind [C] (channel c is of kind c % 8), gamma, beta f32."""
    rng = np.random.RandomState(1000 * M + C)
    kind = np.arange(C) % 8
    y = rng.randn(M, C) * STD
    for c in range(C):
        k = kind[c]
        if k < 5:
            y[:, c] += RATIOS[k] * STD * (1 if (c // 8) % 2 == 0 else -1)
        elif k == KIND_CONST:
            y[:, c] = CONSTANTS[(c // 8) % len(CONSTANTS)]
        elif k == KIND_OUTLIER:
            y[M // 2, c] = 1000.0
        else:
            y[:, c] = 1000.0 + rng.randn(M) * 4.0
    y = inputs64(y.astype(f32), mode).astype(f32)
    y.setflags(write=False)
    gamma = (rng.rand(C) + 0.5).astype(f32) * np.where(np.arange(C) % 5 == 4, -1, 1).astype(f32)
    beta = (rng.randn(C) * 0.2).astype(f32)
    return dict(M=M, C=C, y=y, kind=kind, gamma=gamma, beta=beta)


def placed_shift(y, placement):
    """The f32 shift `placement` away from the batch mean, in units of the channel's std; of 1/3 for a constant channel, so that y - shift is
    no round number there and the rows' rounding is felt."""
    y64 = np.asarray(y, np.float64)
    std = y64.std(0)
    return (y64.mean(0) + PLACEMENTS[placement] * np.where(std > 0, std, 1.0 / 3)).astype(f32)


def fin_combos(M, C):
    """The four (placement, rows) pairs of a shape: every placement once, the rows rotated by the shape's index, so that the twelve shapes
    together launch all sixteen pairs."""
    i = STATS_SHAPES.index((M, C))
    return [(p, FIN_ROWS[(j + i) % 4]) for j, p in enumerate(PLACEMENTS)]


# ------------------------------------------------------------------------------------------------------------------
# conv2d_bn as a producer of partial rows
# ------------------------------------------------------------------------------------------------------------------
CONV_SHAPES = [(2, 13, 13, 64, 64), (1, 26, 26, 32, 64)]        # (B, H, W, Cin, Cout)
CONV_KSIZES = (1, 3)
CONV_MEANS = (0.0, 3.0, 30.0, 300.0)                             # output channel co has mean CONV_MEANS[co % 4] * (-1)^(co // 4), std ~ 1
CONV_SHIFTS = {'mean': 0.0, '30std': 30.0}


@functools.lru_cache(maxsize=None)
def conv_case(shape, k):
    """dict: x [B, H, W, Cin] f32 with channel 0 constant 1, w [k, k, Cin, Cout] f32 whose centre tap of input channel 0 is the chosen mean of
    each output channel (the other taps of that input channel are 0, so the padding does not touch the mean), means [Cout]."""
    B, H, W, Cin, Cout = shape
    rng = np.random.RandomState(sum(shape) + k)
    x = rng.randn(B, H, W, Cin).astype(f32)
    x[..., 0] = 1.0
    w = (rng.randn(k, k, Cin, Cout) / np.sqrt(k * k * (Cin - 1))).astype(f32)
    means = (np.array(CONV_MEANS)[np.arange(Cout) % 4] * np.where((np.arange(Cout) // 4) % 2 == 0, 1, -1)).astype(f32)
    w[:, :, 0, :] = 0
    w[k // 2, k // 2, 0, :] = means
    return dict(x=x, w=w, means=means)


# ------------------------------------------------------------------------------------------------------------------
# B and C. the lattice
# ------------------------------------------------------------------------------------------------------------------
CHANNELS = (8, 16, 24, 40, 48, 96, 136, 192, 320, 520, 1024, 2048)            # 2048: bf16 only (C / vec <= 256)
LATTICE_SHAPES = [(1, 2, 2), (1, 7, 15), (3, 8, 6), (2, 26, 26)]              # M = 4, 105, 144, 1352; all but 7 x 15 have a pooled form
DECISION_CASES = {'d_8x6_40': (2, 8, 6, 40), 'd_8x8_1024': (1, 8, 8, 1024), 'd_12x10_64': (2, 12, 10, 64)}
MUS = (-2.0, -0.5, 0.0, 0.75, 3.0)
DELTAS = (0.125, 0.25, 0.5)
KMAX = 16
WINDOW_KINDS = ('equal', 'tie12', 'tie23', 'distinct')
COLLIDE_EVERY = 7           # bf16 mode: channels c % 7 == 3 are collision channels


def channel_modes(C):
    return [m for m in MODES if C % VEC[m] == 0 and C // VEC[m] <= 256]


def lattice_names():
    """name -> (B, H, W, C, planted): group B by shape and channel count, group C by name."""
    out = {}
    for C in CHANNELS:
        for (B, H, W) in LATTICE_SHAPES:
            out['b_%dx%dx%d_c%d' % (B, H, W, C)] = (B, H, W, C, False)
    for n, (B, H, W, C) in DECISION_CASES.items():
        out[n] = (B, H, W, C, True)
    return out


LATTICE = lattice_names()
LATTICE_RUNS = [(n, m) for n in LATTICE for m in channel_modes(LATTICE[n][3])]


@functools.lru_cache(maxsize=4)
def lattice_case(name, mode):
    """dict: B, H, W, C, M, y [B, H, W, C] f32 with y = mu_c + k delta_c (exact in bf16, so the same tensor in both modes), k (the integers),
    mean (= mu), var, gamma, beta, dgamma_in, dbeta_in f32 [C], da [B, H, W, C] and dp [B, H/2, W/2, C] f32 (multiples of 1/8, exact in
    bf16), fin_s2 [C] f32 (see below), collide [C] bool, planted: window kind -> number of windows planted.
      * gamma is negative in the channels c % 5 == 4;
      * beta is 0 in the channels c % 3 == 0 (z is exactly 0 where k is 0: a stripe of such elements: the first pixel of every second row, or of every
        window that is not planted)
        and 0.37 lattice steps of z elsewhere (|z| >= 0.37 steps, at most 16.37);
      * var is (4 .. 10 delta)^2, but 1e-4 .. 1e-3 in the channels c % 11 == 5 (eps matters there);
      * bf16 mode, channels c % 7 == 3 ("collision channels"): beta = 1 and a lattice step of z of 2^-14, so every activation is within 2^-10
        of 1 and rounds to exactly 1 in bf16 (the nearest rounding boundaries are at 1 - 2^-9 and 1 + 2^-8) while they differ in f32;
      * planted windows (decision cases; window number w of a channel, kind w % 8 < 4): all four equal; equal maxima at positions (1, 2);
        at (2, 3); four distinct values.  "Maximum" is meant of the activation: in a channel with negative gamma the planted k are negated."""
    B, H, W, C, planted = LATTICE[name]
    rng = np.random.RandomState(((B * 131 + H) * 131 + W) * 4099 + C)
    M = B * H * W
    ch = np.arange(C)
    mu = np.array(MUS)[rng.randint(0, len(MUS), C)]
    delta = np.array(DELTAS)[rng.randint(0, len(DELTAS), C)]
    k = rng.randint(-KMAX, KMAX + 1, (B, H, W, C))
    sign = np.where(ch % 5 == 4, -1.0, 1.0)
    gamma = (sign * rng.uniform(0.5, 1.5, C)).astype(f32)
    var = ((delta * rng.uniform(4, 10, C)) ** 2).astype(f32)
    small = ch % 11 == 5
    var[small] = rng.uniform(1e-4, 1e-3, int(small.sum())).astype(f32)
    collide = (ch % COLLIDE_EVERY == 3) & (mode == 'bf16')
    var[collide] = ((delta[collide] * np.abs(gamma[collide].astype(np.float64)) * 2.0 ** 14) ** 2).astype(f32)
    # the variance is one that a finalisation can produce EXACTLY: fin_s2 / M in f64, rounded to f32 (a *_fin consumer given partial rows that
    # sum to 0 in plane 0 and to fin_s2 in plane 1, with shift = mu, normalises with exactly this mean and var)
    fin_s2 = (var.astype(np.float64) * M).astype(f32)
    var = (fin_s2.astype(np.float64) / M).astype(f32)
    step = delta * np.abs(gamma.astype(np.float64)) / np.sqrt(var.astype(np.float64) + EPS)       # |z(k + 1) - z(k)|
    beta = np.where(ch % 3 == 0, 0.0, 0.37 * step * np.where(rng.rand(C) < 0.5, -1.0, 1.0))
    beta[collide] = 1.0
    beta = beta.astype(f32)
    if not planted:
        k[:, ::2, 0, :] = np.where((ch % 3 == 0)[None, None, :], 0, k[:, ::2, 0, :])               # the stripe of exact zeros
    counts = dict.fromkeys(WINDOW_KINDS, 0)
    if planted:
        OW = W // 2
        for b in range(B):
            for oh in range(H // 2):
                for ow in range(OW):
                    kind = ((b * (H // 2) + oh) * OW + ow) % 8
                    if kind >= 4:
                        k[b, 2 * oh, 2 * ow, ch % 3 == 0] = 0                                          # the stripe, in the windows that are not planted
                        continue
                    lo = rng.randint(-KMAX, 0, (4, C))
                    hi = rng.randint(1, KMAX + 1, C)
                    if kind == 0:
                        t = np.broadcast_to(rng.randint(-KMAX, KMAX + 1, C), (4, C)).copy()
                    elif kind == 1:
                        t = np.stack([lo[0], hi, hi, lo[3]])
                    elif kind == 2:
                        t = np.stack([lo[0], lo[1], hi, hi])
                    else:
                        t = np.stack([rng.permutation(2 * KMAX + 1)[:4] - KMAX for _ in range(C)], 1)
                    t = (t * sign[None, :]).astype(np.int64)
                    k[b, 2 * oh:2 * oh + 2, 2 * ow:2 * ow + 2, :] = t.reshape(2, 2, C)
                    counts[WINDOW_KINDS[kind]] += 1
    y = (mu + k * delta).astype(f32)
    assert np.array_equal(R.bf16_round(y), y)
    y.setflags(write=False)
    da = (rng.randint(-8, 9, (B, H, W, C)) / 8.0).astype(f32)
    dp = (rng.randint(-8, 9, (B, H // 2, W // 2, C)) / 8.0).astype(f32) if H % 2 == 0 and W % 2 == 0 else None
    dgamma_in = (rng.randn(C) * np.sqrt(M)).astype(f32)
    dbeta_in = (rng.randn(C) * np.sqrt(M)).astype(f32)
    return dict(name=name, B=B, H=H, W=W, C=C, M=M, y=y, k=k, mean=mu.astype(f32), var=var, gamma=gamma, beta=beta, da=da, dp=dp,
                dgamma_in=dgamma_in, dbeta_in=dbeta_in, fin_s2=fin_s2, collide=collide, planted=counts, pooled=dp is not None)


@functools.lru_cache(maxsize=4)
def lattice_reference(name, mode):
    """float64 references of every kernel on a lattice case.  dict: z, a; g, gx (the summands of dbeta, dgamma over the M pixels), dy (with
    dgamma_in / dbeta_in); where the case has a pooled form: a_st (the activations as stored: rounded to bf16 in bf16 mode), arg uint8
    [B, OH, OW, C] (first maximum of a_st), p (a at arg, unrounded), ymax (y at arg), pg, pgx (the summands of the pooled backward: g and
    g * xhat at the arg-max pixel of the routed dp, [B * OH * OW, C]), pdy [B, H, W, C] (pooled backward with dgamma_in / dbeta_in, count M)."""
    c = lattice_case(name, mode)
    B, H, W, C, M = c['B'], c['H'], c['W'], c['C'], c['M']
    y = c['y'].astype(np.float64)
    par = (c['mean'], c['var'], c['gamma'], c['beta'])
    z, a = fwd64(y, *par)
    g, gx = bwd_terms64(y, c['da'], *par)
    out = dict(z=z, a=a, g=g.reshape(M, C), gx=gx.reshape(M, C), dy=bwd_apply64(y, c['da'], *par, c['dgamma_in'], c['dbeta_in'], M))
    if c['pooled']:
        a_st = stored(a, mode)
        arg = windows(a_st).argmax(0).astype(np.uint8)
        ymax = take(windows(y), arg)
        pg, pgx = bwd_terms64(ymax, c['dp'], *par)
        out.update(a_st=a_st, arg=arg, p=take(windows(a), arg), ymax=ymax, pg=pg.reshape(-1, C), pgx=pgx.reshape(-1, C),
                   pdy=bwd_apply64(y, route(c['dp'].astype(np.float64), arg), *par, c['dgamma_in'], c['dbeta_in'], M))
    return out


def conditions(name, mode):
    """The decision-point conditions of a lattice case, over EVERY element and EVERY window.  dict: zmargin (the smallest non-zero |z| over the
    channel's largest), zeros (elements with z exactly 0), neg_zero (of those, with a negative gamma), window counts by kind ('equal': all
    four stored activations equal; 'tie12' / 'tie23': exactly two equal maxima at those positions; 'distinct'; 'collision': bf16 only,
    the two best stored activations are bit-equal while the later one is larger in f32), gap: the smallest separation of the two best
    activations of any window where they are not bit-equal after the store's rounding, in units of the threshold (four bf16 ulps of the
    larger one in bf16 mode, 1e-3 relative in f32 mode)."""
    c, ref = lattice_case(name, mode), lattice_reference(name, mode)
    z = ref['z'].reshape(c['M'], c['C'])
    az = np.abs(z)
    zmax = az.max(0)
    nz = np.where(az > 0, az / zmax, np.inf)
    out = dict(zmargin=float(nz.min()), zeros=int((z == 0).sum()), neg_zero=int(((z == 0) & (c['gamma'] < 0)[None, :]).sum()))
    if c['pooled']:
        w64, wst = windows(ref['a']), windows(ref['a_st'])
        order = np.argsort(-wst, axis=0, kind='stable')
        first, second = order[0], order[1]
        top_st, sec_st = take(wst, first), take(wst, second)
        top, sec = take(w64, first), take(w64, second)
        equal = top_st == sec_st
        thr = (4 * BF16_ULP if mode == 'bf16' else MARGIN) * np.maximum(np.abs(top), np.abs(sec))
        with np.errstate(divide='ignore', invalid='ignore'):
            gap = np.where(equal, np.inf, (top - sec) / thr)
        nmax = (wst == wst.max(0)[None]).sum(0)
        pos = [(wst[p] == wst.max(0)) for p in range(4)]
        out.update(gap=float(gap.min()), equal=int((nmax == 4).sum()), tie12=int(((nmax == 2) & pos[1] & pos[2]).sum()),
                   tie23=int(((nmax == 2) & pos[2] & pos[3]).sum()), distinct=int((nmax == 1).sum()),
                   collision=int((equal & (w64.argmax(0) > first)).sum()))
    return out
