"""yolo2_grad_combine on the device against the NumPy specification (tests/grad_combine_ref.py), bit for bit: every mode, sizes around the 16-byte group and
the workgroup chunk, range tables with arbitrary begins and ends, special values at the range edges, guard bands, misaligned arenas, argument errors.

NaN is compared by position (the payload of a NaN that an addition produces is not part of IEEE arithmetic and differs between the host and the device), every other
value -- infinities, signed zeros and denormals included -- by its 32 bits, as tests/test_ema_gpu.py does."""
import itertools

import numpy as np
import pytest
import torch

import grad_combine_ref as ref

pytestmark = pytest.mark.gpu

CHUNK = 4096                                                          # YOLO2_GRAD_COMBINE_CHUNK
SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7]
SCALES = [1.0, float(np.float32(1.0 / 3.0)), 1.0 / 8.0]
DECAYS = [0.0, 5e-4]
SHRINKS = [1.0, float(np.float32(1.0 - 1e-3 * 5e-4))]
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-41], np.float32)     # (1e-41: a denormal)
SENTINEL = np.float32(12345.0)
GUARD = 8                                                             # elements on either side of every arena of every case
# element offsets of (g, acc, w) from a 16-byte boundary: aligned; all three shifted alike (`arena[1:]`: still 16-byte accesses behind a scalar head); acc
# alone shifted and w alone shifted (the arenas are then not aligned alike: scalar accesses)
ALIGNMENTS = [(0, 0, 0), (1, 1, 1), (0, 1, 0), (2, 2, 3)]


def test_the_chunk_constant_is_the_librarys():
    import os
    import re
    from yolo_tf_amd import ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'yolo2_hip.h')).read()
    assert int(re.search(r'#define YOLO2_GRAD_COMBINE_CHUNK (\d+)', header).group(1)) == CHUNK == ops.GRAD_COMBINE_CHUNK
    assert (ops.GRAD_STORE, ops.GRAD_ADD, ops.GRAD_FINAL) == (ref.STORE, ref.ADD, ref.FINAL)


def tables(n):
    """The range tables for an arena of n elements: empty; the whole arena; begins and ends that are no multiples of 4, two adjacent ranges, a range of length 1
    and a range that ends at n; a range across a chunk boundary; whole chunks (inside one range from end to end); 300 ranges within two chunks."""
    t = [[]]
    if n >= 1:
        t.append([(0, n)])
        t.append([(n - 1, n)])
    if 3 <= n < 16:
        t.append([(1, 2), (2, n)])
    if n >= 16:
        t.append([(1, 3), (5, 6), (6, 11), (13, 14), (n - 3, n)])
    if n > CHUNK + 6:
        t.append([(CHUNK - 5, CHUNK + 6)])
    if n >= 3 * CHUNK:
        t.append([(3, CHUNK), (CHUNK, 2 * CHUNK + 1), (3 * CHUNK - 1, n - 1)])
        t.append([(27 * k + 1, 27 * k + 2 + k % 25) for k in range(300)])
        assert t[-1][-1][1] <= 2 * CHUNK
    return t


def _bits_equal_nan_by_position(got, want):
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(got.view(np.int32)[~gn], want.view(np.int32)[~wn])


_NOISE = []


def _inputs(n, k, ranges):
    """Three windows of fixed noise (drawn once) at magnitudes a gradient, its running sum and a weight have, the special values planted at the range edges
    (and at the arena's own edges), a different arena taking each special in every case."""
    if not _NOISE:
        rng = np.random.RandomState(11)
        _NOISE.extend(rng.standard_normal(max(SIZES) + 8192).astype(np.float32) for _ in range(3))
    arenas = [_NOISE[a][(3 + 2 * a) * (k % 1024):][:n] * np.float32(s) for a, s in enumerate((1e-2, 3e-2, 0.5))]
    if n:
        edges = sorted(set([0, n - 1] + [i for b, e in ranges[:8] for i in (b - 1, b, e - 1, e) if 0 <= i < n]))
        for j, i in enumerate(edges):
            arenas[(j + k) % 3][i] = SPECIALS[(j + k // 3) % len(SPECIALS)]
    return arenas


def _cases(n):
    out = [(mode, True, 1.0, 0.0, 1.0, []) for mode in (ref.STORE, ref.ADD)]
    for has_acc, scale, decay, shrink, table in itertools.product((True, False), SCALES, DECAYS, SHRINKS, tables(n)):
        out.append((ref.FINAL, has_acc, scale, decay, shrink, table))
    if n <= 1025:
        return [c + (al,) for c in out for al in ALIGNMENTS]
    # the larger sizes: the alignments taken in turn (the tables vary fastest and their count is odd or coprime enough that every table meets every alignment)
    out = [c + (ALIGNMENTS[(k + k // len(ALIGNMENTS)) % len(ALIGNMENTS)],) for k, c in enumerate(out)]
    return out + [(mode, True, 1.0, 0.0, 1.0, [], al) for mode in (ref.STORE, ref.ADD) for al in ALIGNMENTS[1:]]


@pytest.mark.parametrize('n', SIZES)
def test_kernel_equals_the_specification_bit_for_bit(n):
    """Every case in a slot of its own of three big buffers (g, acc, w): sentinels, the case's misalignment, the n elements, sentinels.  One upload, one launch
    per case, one download; the whole buffers are compared, so the guard bands and every element outside the ranges must keep their bits."""
    from yolo_tf_amd import ops
    cases = _cases(n)
    slot = (n + 2 * GUARD + 4 + 3) // 4 * 4
    host = [np.full(slot * len(cases), SENTINEL, np.float32) for _ in range(3)]
    want = [h.copy() for h in host]
    where = []
    for k, (mode, has_acc, scale, decay, shrink, table, al) in enumerate(cases):
        g, acc, w = _inputs(n, k, table)
        at = [k * slot + GUARD + o for o in al]
        for h, a, x in zip(host, at, (g, acc, w)):
            h[a:a + n] = x
        rg, racc, rw = ref.combine(g, acc if (has_acc or mode != ref.FINAL) else None, w, mode, scale, decay, shrink, table)
        for x, a, r, orig in zip(want, at, (rg, racc, rw), (g, acc, w)):
            x[a:a + n] = orig if r is None else r
        where.append(at)
    dev = [torch.from_numpy(h).cuda() for h in host]
    assert all(d.data_ptr() % 16 == 0 for d in dev)
    filler = torch.zeros(4, dtype=torch.float32, device='cuda')         # (n = 0: an empty view has no address to pass)
    for (mode, has_acc, scale, decay, shrink, table, al), at in zip(cases, where):
        g, acc, w = [d[a:a + n] if n else filler for d, a in zip(dev, at)]
        tab = ops.grad_ranges(table, n, 'cuda')
        ops.grad_combine(g, acc if (has_acc or mode != ref.FINAL) else None, w, n, mode, scale, decay, shrink, tab)
    got = [d.cpu().numpy() for d in dev]
    for name, x, y in zip(('g', 'acc', 'w'), got, want):
        if not _bits_equal_nan_by_position(x, y):
            for k, case in enumerate(cases):
                s = slice(k * slot, (k + 1) * slot)
                assert _bits_equal_nan_by_position(x[s], y[s]), '%s: n = %d, (mode, acc, scale, decay, shrink, ranges, alignment) = %r' % (name, n, case)
    if n >= 16:      # the arithmetic was exercised: decay moved some gradient, shrink some weight, and only inside the ranges
        assert any(not np.array_equal(got[2][k * slot:(k + 1) * slot], host[2][k * slot:(k + 1) * slot]) for k, c in enumerate(cases) if c[4] != 1.0 and c[5])
        assert all(np.array_equal(got[2][k * slot:(k + 1) * slot].view(np.int32), host[2][k * slot:(k + 1) * slot].view(np.int32))
                   for k, c in enumerate(cases) if c[4] == 1.0 or not c[5])


def test_a_chunk_inside_one_range_and_the_general_path_agree():
    """The same arena through the 16-byte path (aligned alike) and the scalar path (w shifted by one element): the same bits."""
    from yolo_tf_amd import ops
    n = 3 * CHUNK + 7
    g, acc, w = _inputs(n, 5, [(0, n)])
    table = [(3, 2 * CHUNK + 1), (2 * CHUNK + 1, n)]
    out = []
    for shift in (0, 1):
        dg, dacc = torch.from_numpy(g).cuda(), torch.from_numpy(acc).cuda()
        dw = torch.from_numpy(np.concatenate([np.zeros(shift, np.float32), w])).cuda()[shift:]
        ops.grad_combine(dg, dacc, dw, n, ops.GRAD_FINAL, SCALES[1], DECAYS[1], SHRINKS[1], ops.grad_ranges(table, n, 'cuda'))
        out.append((dg.cpu().numpy(), dw.cpu().numpy()))
    assert _bits_equal_nan_by_position(out[0][0], out[1][0]) and _bits_equal_nan_by_position(out[0][1], out[1][1])
    rg, _, rw = ref.combine(g, acc, w, ref.FINAL, SCALES[1], DECAYS[1], SHRINKS[1], table)
    assert _bits_equal_nan_by_position(out[0][0], rg) and _bits_equal_nan_by_position(out[0][1], rw)


def test_argument_errors_come_back_through_the_c_abi():
    from yolo_tf_amd import _lib, ops
    x = torch.zeros(64, dtype=torch.float32, device='cuda')
    y, z = torch.ones_like(x), torch.ones_like(x)
    table = ops.grad_ranges([(0, 8)], 64, 'cuda')
    bad = [
        lambda: ops.grad_combine(x, y, z, -1, ops.GRAD_ADD),                                         # n < 0
        lambda: ops.grad_combine(x, y, z, 64, 3),                                                     # an unknown mode
        lambda: ops.grad_combine(x, y, z, 64, -1),
        lambda: ops.grad_combine(x, None, z, 64, ops.GRAD_STORE),                                     # no accumulator to store into / add to
        lambda: ops.grad_combine(x, None, z, 64, ops.GRAD_ADD),
        lambda: ops.grad_combine(x, y, None, 64, ops.GRAD_FINAL, 1.0, 5e-4, 1.0, table),              # decays without the weights
        lambda: ops.grad_combine(x, y, None, 64, ops.GRAD_FINAL, 1.0, 0.0, 0.5, table),
        lambda: _lib.call('yolo2_grad_combine', x.data_ptr(), y.data_ptr(), z.data_ptr(), 64, 2, 1.0, 5e-4, 1.0, None, 1, None),      # ... or the table
        lambda: _lib.call('yolo2_grad_combine', x.data_ptr(), y.data_ptr(), z.data_ptr(), 64, 2, 1.0, 0.0, 0.5, None, 1, None),
        lambda: _lib.call('yolo2_grad_combine', x.data_ptr(), y.data_ptr(), z.data_ptr(), 64, 2, 1.0, 0.0, 1.0, None, -1, None),      # n_ranges < 0
        lambda: ops.grad_combine(None, None, z, 64, ops.GRAD_FINAL),                                  # no gradient
    ]
    for f in bad:
        with pytest.raises(_lib.HipKernelError, match='argument check failed'):
            f()
    # the table's order is checked where it is built, on the host
    for ranges in ([(8, 4)], [(4, 4)], [(0, 65)], [(-1, 3)], [(8, 16), (0, 4)], [(0, 8), (7, 12)]):
        with pytest.raises(ValueError, match='grad_combine'):
            ops.grad_ranges(ranges, 64, 'cuda')
    assert ops.grad_ranges([], 64, 'cuda') is None and ops.grad_ranges([(0, 8), (8, 64)], 64, 'cuda').tolist() == [0, 8, 8, 64]
    # nothing above was launched; what is allowed: no decay asked for, so neither w nor the table is needed
    ops.grad_combine(x, y, None, 64, ops.GRAD_FINAL, 0.5, 0.0, 1.0, table)
    ops.grad_combine(x, y, None, 0, ops.GRAD_FINAL, 0.5, 5e-4, 1.0, None)
    torch.cuda.synchronize()
    assert torch.equal(x, torch.full_like(x, 0.5)) and torch.equal(y, torch.ones_like(y)) and torch.equal(z, torch.ones_like(z))
