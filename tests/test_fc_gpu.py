"""The fully connected shapes of the YOLO (v1) family on the device: 1x1 convolutions with 1 to 8 rows (H = W = 1, M = B) through ops.conv2d,
ops.conv2d_ws and ops.conv2d_bias_leaky, their filter gradients (ops.conv2d_wgrad) and bias gradients (ops.bias_grad), in f32 and bf16 against the
float64 oracle on exactly the values they read -- the cases, references and bounds of tests/fc_cases.py, whose own conditions, the launch rule's
answer for each and the proof that the bounds catch a subtly wrong kernel are in tests/test_fc_cases_cpu.py -- and the three element-wise kernels only
this family uses (csrc/yolo1.hip: leaky_bwd, dropout / dropout_bwd, l2_regularizer) bit for bit at the sizes where their loops take another turn.

Every launch is guarded: operands and outputs live in the middle of a larger allocation whose ends are filled with NaN (0xA5 bytes for a mask), an
output starts out as NaN with zero padding lanes and is followed by a whole tile's worth of guard rows, the workspace is NaN.  After the launch the
real rows are finite and inside the bound, the padding lanes are still zero, every guard element still holds its bit pattern, every operand is what it
was, and the plan word names the branch the case is named for.  A correct kernel never touches a guard; a read or a store past row M fails here.

`pytest -s` prints one `fc-shapes |` line per launch: case, dtype, epilogue, route, worst |err| / bound (profiles/fc_shapes.md)."""
import numpy as np
import pytest
import torch

import fc_cases as F
from oracle import yolo2_ref as R
import test_kernels_gpu as K

pytestmark = pytest.mark.gpu

assert (K.F32_RTOL, K.WGRAD_REL, K.WGRAD_FLOOR) == (F.F32_RTOL, F.WGRAD_REL, F.WGRAD_FLOOR)      # fc_cases restates no bound of its own
TDTYPE = {'f32': torch.float32, 'bf16': torch.bfloat16}
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64, torch.uint8: torch.uint8}
GUARD_BYTES = 1024        # a multiple of 16: the guarded pointers stay 16-byte aligned
TILE_ROWS = 128
FWD_RUNS = [(n, m, e, True) for n in F.FWD_SPECS for m in F.MODES for e in F.EPILOGUES] + \
           [(n, m, e, False) for n in F.FWD_SPECS for m in F.MODES for e in F.EPILOGUES if F.sliced(n, m)]
SLICED = [(n, m) for n in F.FWD_SPECS for m in F.MODES if F.sliced(n, m)]


@pytest.fixture(scope='module')
def ops():
    from yolo_tf_amd import ops as _ops
    _ops._lib.load()
    assert torch.cuda.is_available()
    print('fc-shapes | device: %s, %d CUs' % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count))
    return _ops


# ---------------------------------------------------------------------------------------------------------------------
# bit-level transfers (no conversion runs on the device) and guarded buffers
# ---------------------------------------------------------------------------------------------------------------------

def to_device(x, dtype):
    """np f32 values -> device tensor of `dtype`; bf16: rounded to nearest even on the host, uploaded as bits."""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == torch.float32:
        return torch.from_numpy(x.reshape(-1).copy()).cuda()
    assert dtype == torch.bfloat16
    bits = (R.bf16_round(x).view(np.uint32) >> 16).astype(np.uint16).reshape(-1)
    return torch.from_numpy(bits.view(np.int16).copy()).cuda().view(torch.bfloat16)


def to_host(t):
    """Device tensor -> np f32 holding exactly the stored values (bf16: its 16 bits widened on the host)."""
    if t.dtype == torch.bfloat16:
        bits = t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).astype(np.uint32) << 16
        return bits.view(np.float32)
    return t.cpu().numpy()


def bits_of(x, dtype):
    """The stored bits of np f32 values in `dtype` (bf16: after round-to-nearest-even)."""
    x = np.ascontiguousarray(x, np.float32)
    return x.view(np.uint32) if dtype == torch.float32 else (R.bf16_round(x).view(np.uint32) >> 16)


class Guarded(object):
    """`n` elements of `dtype` in the middle of a larger allocation: GUARD_BYTES before, at least as much (`after` elements) behind, both filled
    with NaN (0xA5 for bytes).  `fill`: a device tensor or a scalar for the body, else NaN too.  arm() before the launch, check() after it."""

    def __init__(self, n, dtype, fill=None, after=0):
        esz = torch.empty((), dtype=dtype).element_size()
        self.n, self.front, self.dtype = int(n), GUARD_BYTES // esz, dtype
        back = max(GUARD_BYTES // esz, int(after))
        self.poison = 0xA5 if dtype == torch.uint8 else float('nan')
        self.buf = torch.full((self.front + self.n + back,), self.poison, dtype=dtype, device='cuda')
        self.t = self.buf[self.front:self.front + self.n]
        assert self.t.data_ptr() % 16 == 0 and self.t.is_contiguous()
        if fill is not None:
            self.set(fill)
        self.snapshot = None

    def set(self, fill):
        if torch.is_tensor(fill):
            self.t.copy_(fill.reshape(-1))
        else:
            self.t.fill_(fill)

    def poison_all(self):
        self.buf.fill_(self.poison)

    def arm(self):
        self.snapshot = self.buf.view(INT_VIEW[self.dtype]).clone()
        return self.t

    def check(self, what, readonly=False):
        now, was = self.buf.view(INT_VIEW[self.dtype]), self.snapshot
        a, b = self.front, self.front + self.n
        assert torch.equal(now[:a], was[:a]), '%s: the guard BEFORE the buffer was written' % what
        if not torch.equal(now[b:], was[b:]):
            first = int(torch.nonzero(now[b:] != was[b:])[0])
            raise AssertionError('%s: the guard BEHIND the buffer was written, first at element +%d' % (what, first))
        if readonly:
            assert torch.equal(now[a:b], was[a:b]), '%s: an operand was written' % what


_WS = {}


def workspace():
    """The session's 32 MiB workspace, guarded, NaN everywhere (one allocation for the module)."""
    if 'ws' not in _WS:
        _WS['ws'] = Guarded(F.WS_FLOATS, torch.float32)
    _WS['ws'].poison_all()
    return _WS['ws']


def report(case, mode, epilogue, route, ratio):
    print('fc-shapes | %s | %s | %s | %s | %.3f' % (case, mode, epilogue, route, ratio))


# ---------------------------------------------------------------------------------------------------------------------
# forward and data gradient
# ---------------------------------------------------------------------------------------------------------------------

def fwd_operands(ops, name, mode):
    """(P guarded [B, Cp], F guarded: the filter as filter_prep lays it out, bias guarded f32) of a case, on the device."""
    c, T = F.fwd_case(name), TDTYPE[mode]
    B, Cp, C, Nf = c['B'], F.FWD_SPECS[name][1], c['C'], c['Nf']
    x, w = F.inputs64(c['x'], mode).astype(np.float32), F.inputs64(c['w'], mode).astype(np.float32)
    P = Guarded(B * Cp, T, to_device(K.pad_channels(x, Cp), T))
    Ff = Guarded(Nf * Cp, T, 0.0)
    if c['kind'] == 'dgrad':      # W in HWIO = [1, 1, Nf, C]; the transposed output of filter_prep is the data gradient's filter (tests/test_kernels_gpu.py test_conv_dgrad)
        ops.filter_prep(to_device(w.T, torch.float32), None, Ff.t, 1, Nf, F.pad8(Nf), C, Cp, T)
    else:
        ops.filter_prep(to_device(w, torch.float32), Ff.t, None, 1, C, Cp, Nf, F.pad8(Nf), T)
    bias = Guarded(Nf, torch.float32, to_device(c['bias'], torch.float32))
    torch.cuda.synchronize()
    return P, Ff, bias


def fwd_launch(ops, name, mode, epilogue, with_ws, operands):
    """One guarded launch.  -> (rows [B, ldo] as np f32, plan)."""
    c, T = F.fwd_case(name), TDTYPE[mode]
    B, Cp, Nf, ldo = c['B'], F.FWD_SPECS[name][1], c['Nf'], c['ldo']
    P, Ff, bias = operands
    O = Guarded(B * ldo, T, after=TILE_ROWS * ldo)
    O.t.view(B, ldo)[:, Nf:] = 0            # the padding lanes, as run_conv pre-sets them
    ws = workspace() if with_ws else None
    bufs = [('P', P, True), ('F', Ff, True), ('bias', bias, True), ('O', O, False)] + ([('ws', ws, False)] if ws else [])
    for _, g, _ in bufs:
        g.arm()
    bt = None if epilogue == 'plain' else bias.t
    wt = ws.t if ws else None
    if epilogue == 'bias_leaky':
        ops.conv2d_bias_leaky(P.t, Ff.t, bt, O.t, wt, B, 1, 1, Cp, Cp, Nf, ldo, 1, F.ALPHA)
    elif with_ws:
        ops.conv2d_ws(P.t, Ff.t, bt, O.t, wt, B, 1, 1, Cp, Cp, Nf, ldo, 1)
    else:
        ops.conv2d(P.t, Ff.t, bt, O.t, B, 1, 1, Cp, Cp, Nf, ldo, 1)
    torch.cuda.synchronize()
    plan = ops.last_conv_plan()
    what = 'fc %s %s %s ws=%d' % (name, mode, epilogue, with_ws)
    for label, g, readonly in bufs:
        g.check('%s, %s' % (what, label), readonly)
    return to_host(O.t).reshape(B, ldo), plan


def check_rows(rows, name, mode, epilogue, plan, want, what):
    c = F.fwd_case(name)
    Nf = c['Nf']
    assert F.branch_of(plan) == want, (what, plan)
    got, ref = rows[:, :Nf], F.fwd_reference(name, mode, epilogue)['y']
    assert np.all(np.isfinite(got)), '%s: %d of %d real elements were not written (or are not finite)' % (what, int((~np.isfinite(got)).sum()), got.size)
    assert np.all(rows[:, Nf:] == 0), '%s: padding lanes' % what
    ratio = F.out_ratio(got, ref, mode)
    report(name, mode, epilogue, '%s %dx%d' % (want, plan['grid_x'], plan['grid_y']), ratio)
    assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize('name,mode,epilogue,with_ws', FWD_RUNS, ids=['%s-%s-%s-%s' % (n, m, e, 'ws' if w else 'nows') for n, m, e, w in FWD_RUNS])
def test_fc_forward(ops, name, mode, epilogue, with_ws):
    c = F.fwd_case(name)
    rows, plan = fwd_launch(ops, name, mode, epilogue, with_ws, fwd_operands(ops, name, mode))
    # the branch the case is named for, and what the pure rule answers for this device's own CU count
    route = ops.conv_route(c['B'], 1, 1, F.FWD_SPECS[name][1], F.FWD_SPECS[name][1], c['Nf'], c['ldo'], 1, TDTYPE[mode], 'plain' if epilogue == 'plain' else 'bias_act',
                           4 * F.WS_FLOATS if with_ws else 0)
    assert plan == route['plan'], (plan, route)
    check_rows(rows, name, mode, epilogue, plan, F.expected_branch(name, mode, with_ws), 'fc %s %s %s ws=%d' % (name, mode, epilogue, with_ws))


@pytest.mark.parametrize('name,mode', SLICED)
def test_fc_forward_deterministic_mode_refuses_k_slices(ops, name, mode):
    """ops.set_deterministic(1): the rule names no K slicing (its slices meet in f32 atomics); two launches are bit-identical."""
    operands = fwd_operands(ops, name, mode)
    ops.set_deterministic(1)
    try:
        rows1, plan1 = fwd_launch(ops, name, mode, 'bias_leaky', True, operands)
        rows2, plan2 = fwd_launch(ops, name, mode, 'bias_leaky', True, operands)
    finally:
        ops.set_deterministic(0)
    assert plan1 == plan2 and plan1['split'] == 0 and plan1['grid_y'] == 1, (plan1, plan2)
    assert np.array_equal(rows1.view(np.uint32), rows2.view(np.uint32))
    check_rows(rows1, name, mode, 'bias_leaky', plan1, F.expected_branch(name, mode, True, deterministic=True), 'fc %s %s deterministic' % (name, mode))


# ---------------------------------------------------------------------------------------------------------------------
# filter gradient and bias gradient
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(F.WGRAD_SPECS))
@pytest.mark.parametrize('mode', F.MODES)
def test_fc_filter_gradient(ops, name, mode):
    c, T = F.wgrad_case(name), TDTYPE[mode]
    B, Cin, Cout = c['B'], c['Cin'], c['Cout']
    ldx, ldy = F.pad8(Cin), F.pad8(Cout)
    assert not ops.conv2d_wgrad_accumulates(B, 1, 1, Cin, ldx, Cout, ldy, 1, T)
    X = Guarded(B * ldx, T, to_device(K.pad_channels(F.inputs64(c['x'], mode).astype(np.float32), ldx), T))
    dY = Guarded(B * ldy, T, to_device(K.pad_channels(F.inputs64(c['dy'], mode).astype(np.float32), ldy), T))
    dW = Guarded(Cin * Cout, torch.float32, 123.0)          # dirty on purpose: a single pixel range stores
    for g in (X, dY, dW):
        g.arm()
    ops.conv2d_wgrad(X.t, dY.t, dW.t, B, 1, 1, Cin, ldx, Cout, ldy, 1)
    torch.cuda.synchronize()
    plan = ops.last_wgrad_plan()
    what = 'fc wgrad %s %s' % (name, mode)
    X.check(what + ', X', True), dY.check(what + ', dY', True), dW.check(what + ', dW')
    tile = 64 if name == 'w_b1_c520' else 128
    assert (plan['BC'], plan['BN'], plan['ranges'], plan['direct']) == (tile, tile, 1, 1) and plan['blocks'] == -(-Cin // tile) * -(-Cout // tile), plan
    got, ref = to_host(dW.t).reshape(Cin, Cout), F.wgrad_reference(name, mode)
    assert np.all(np.isfinite(got)), what
    report(name, mode, 'wgrad', 'per-tap %dx%d tile, %d blocks' % (tile, tile, plan['blocks']), F.wgrad_ratio(got, ref, mode))
    if mode == 'f32':
        K.assert_close(got, ref, K.F32_RTOL, what)
    else:
        K.assert_wgrad_exact_products(got, ref, what)
        if B == 1:      # one exact product per element, every other summand of the reduction tile an exact zero
            assert np.array_equal(got.astype(np.float64), ref), '%s: %d elements differ from the exact product' % (what, int((got != ref).sum()))


@pytest.mark.parametrize('name', list(F.BIAS_GRAD_SPECS))
@pytest.mark.parametrize('mode', F.MODES)
def test_fc_bias_gradient(ops, name, mode):
    c, T = F.bias_grad_case(name), TDTYPE[mode]
    M, C, ld = c['M'], c['C'], c['ld']
    dY = Guarded(M * ld, T, to_device(K.pad_channels(F.inputs64(c['dy'], mode).astype(np.float32), ld), T))
    db = Guarded(C, torch.float32)
    ws = Guarded(int(ops._lib.query('yolo2_bias_grad_workspace_bytes', ld)) // 8, torch.float64)
    for g in (dY, db, ws):
        g.arm()
    ops.bias_grad(dY.t, ld, db.t, ws.t, M, C)
    torch.cuda.synchronize()
    what = 'fc bias_grad %s %s' % (name, mode)
    dY.check(what + ', dY', True), db.check(what + ', dbias'), ws.check(what + ', ws')
    got, ref = to_host(db.t), F.bias_grad_reference(name, mode)
    assert np.all(np.isfinite(got)), what
    report(name, mode, 'bias_grad', 'thread per column' if ld // (8 if mode == 'bf16' else 4) > 256 else 'workgroup per 16 bytes', F.f32_ratio(got, ref))
    K.assert_close(got, ref, K.F32_RTOL, what)


# ---------------------------------------------------------------------------------------------------------------------
# csrc/yolo1.hip: leaky_bwd, dropout / dropout_bwd, l2_regularizer
# ---------------------------------------------------------------------------------------------------------------------
GRID_THREADS = 2048 * 256        # the three kernels' largest grid: more elements (vectors) than this take a second turn of the grid-stride loop
SUBNORMAL = {'f32': 2.0 ** -149, 'bf16': 2.0 ** -133}
SPECIALS = lambda mode: np.array([0.0, -0.0, SUBNORMAL[mode], -SUBNORMAL[mode]], np.float32)


def assert_bits_equal(got_t, want_f32, what):
    """The device tensor holds exactly the values `want_f32` stored in its dtype: every bit, the sign of a zero included."""
    got = got_t.contiguous().view(INT_VIEW[got_t.dtype]).cpu().numpy()
    got = got.view(np.uint16).astype(np.uint32) if got_t.dtype == torch.bfloat16 else got.view(np.uint32)
    want = bits_of(want_f32, got_t.dtype).reshape(-1)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, '%s: %d of %d elements differ, the first at %d: got bits %#x, want %#x' % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize('mode', F.MODES)
@pytest.mark.parametrize('vectors', [1, GRID_THREADS + 77])
def test_leaky_bwd_bit_exact(ops, mode, vectors):
    """dz = a >= 0 ? g : alpha * g in f32 on the stored values; -0.0 and +0.0 take the first branch, the smallest subnormals the branch of their sign."""
    T, vec = TDTYPE[mode], 8 if mode == 'bf16' else 4
    n = vec * vectors
    rng = np.random.RandomState(vectors % 1000 + vec)
    a, g = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    sp = SPECIALS(mode)
    for at in {0, n - 4, max(0, vec * GRID_THREADS - 2), max(0, n // 2)}:      # the first vector, the last, the seam of the loop's two turns, the middle
        if at + 4 <= n:
            a[at:at + 4] = sp
    if mode == 'bf16':
        a, g = R.bf16_round(a), R.bf16_round(g)
    assert np.count_nonzero(a == 0) >= 2 and np.signbit(a[a == 0]).any() and not np.signbit(a[a == 0]).all()
    A, G, Z = Guarded(n, T, to_device(a, T)), Guarded(n, T, to_device(g, T)), Guarded(n, T)
    assert_bits_equal(A.t, a, 'upload')                                          # the subnormals and the signed zeros arrived as they are
    for b in (A, G, Z):
        b.arm()
    ops.leaky_bwd(A.t, G.t, Z.t, n, F.ALPHA)
    torch.cuda.synchronize()
    what = 'leaky_bwd %s n=%d' % (mode, n)
    A.check(what + ', a', True), G.check(what + ', g', True), Z.check(what + ', dz')
    assert_bits_equal(Z.t, np.where(a >= 0, g, np.float32(F.ALPHA) * g), what)


@pytest.mark.parametrize('mode', F.MODES)
@pytest.mark.parametrize('keep_prob', [1.0, 0.5, 0.1])
@pytest.mark.parametrize('n', [1, 255, GRID_THREADS + 3])
def test_dropout_forward_backward(ops, mode, keep_prob, n):
    T = TDTYPE[mode]
    rng = np.random.RandomState(n % 1000 + int(keep_prob * 10))
    x, g = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    if mode == 'bf16':
        x, g = R.bf16_round(x), R.bf16_round(g)
    inv = np.float32(1.0) / np.float32(keep_prob)
    scaled = lambda v, m: np.where(m != 0, v * inv, np.float32(0.0)).astype(np.float32)       # (T)(x * (1.0f / keep_prob)) where kept, +0 elsewhere
    what = 'dropout %s keep %.1f n=%d' % (mode, keep_prob, n)
    X, Gd = Guarded(n, T, to_device(x, T)), Guarded(n, T, to_device(g, T))

    def run(seed, mask_in=None):
        Y, Mk = Guarded(n, T), Guarded(n, torch.uint8, mask_in)
        for b in (X, Y, Mk):
            b.arm()
        ops.dropout(X.t, Y.t, Mk.t, n, keep_prob, seed)
        torch.cuda.synchronize()
        X.check(what + ', x', True), Y.check(what + ', y'), Mk.check(what + ', mask', readonly=seed == 0)
        return Y, Mk.t.cpu().numpy(), Mk

    Y, mask, Mk = run(12345)
    assert set(np.unique(mask).tolist()) <= {0, 1}, np.unique(mask)
    assert_bits_equal(Y.t, scaled(x, mask), what)
    if keep_prob == 1.0:
        assert mask.all()
    _, again, _ = run(12345)
    assert np.array_equal(mask, again)
    _, other, _ = run(12346)
    if n > GRID_THREADS:
        band = lambda p: 4 * np.sqrt(p * (1 - p) / n)
        keep, q = float(mask.mean()), 2 * keep_prob * (1 - keep_prob)
        differ = float((mask != other).mean())
        print('%s: keep rate %.5f (band %.5f), masks of two seeds differ in %.5f (expected %.5f, band %.5f)' % (what, keep, band(keep_prob), differ, q, band(q)))
        assert abs(keep - keep_prob) <= band(keep_prob)
        assert abs(differ - q) <= band(q)
    # seed 0: the mask is an input, read as it is and left as it is
    given = (rng.rand(n) < 0.5).astype(np.uint8)
    Y0, after, _ = run(0, torch.from_numpy(given).cuda())
    assert np.array_equal(after, given)
    assert_bits_equal(Y0.t, scaled(x, given), what + ' given mask')
    # backward: the same masking of the incoming gradient
    DX = Guarded(n, T)
    for b in (Gd, Mk, DX):
        b.arm()
    ops.dropout_bwd(Gd.t, Mk.t, DX.t, n, keep_prob)
    torch.cuda.synchronize()
    Gd.check(what + ', dy', True), Mk.check(what + ', mask (backward)', True), DX.check(what + ', dx')
    assert_bits_equal(DX.t, scaled(g, mask), what + ' backward')


@pytest.mark.parametrize('n', [1, 100003])
def test_l2_regularizer_adds_to_gradient_and_loss(ops, n):
    rng = np.random.RandomState(n % 1000)
    w, g0, scale = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32), 0.001
    term = 0.5 * float(np.float32(scale)) * float((w.astype(np.float64) ** 2).sum())      # (the scale is an f32 argument)
    loss0 = 0.75 * term
    W, G = Guarded(n, torch.float32, to_device(w, torch.float32)), Guarded(n, torch.float32, to_device(g0, torch.float32))
    L = Guarded(1, torch.float64, loss0)
    for b in (W, G, L):
        b.arm()
    ops.l2_regularizer(W.t, G.t, n, scale, L.t)
    torch.cuda.synchronize()
    what = 'l2_regularizer n=%d' % n
    W.check(what + ', w', True), G.check(what + ', g'), L.check(what + ', loss')
    loss = float(L.t.cpu()[0])
    assert np.allclose(to_host(G.t), g0 + np.float32(scale) * w)
    assert abs(loss - (loss0 + term)) < 1e-6 * loss, (loss, loss0, term)
