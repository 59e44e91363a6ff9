"""csrc/optim.hip on the cases of tests/optim_cases.py: the seven optimizers step by step against the float64 oracle on exactly the state the
device holds before each step (12 steps, gradient scales 1, 1/3, 1/8, sizes 1 .. 10007, gradients over twelve decades with exact zeros,
squares that underflow and sqrt(v) ~ eps), Adam's scalar path (misaligned arenas), its strided loop and arena slices that are no multiple
of 4; clip_by_norm and clip_by_norm_fixed on one table of segment lengths and contents (early return, zero, empty and overflowing segments,
inf and NaN); zero_ranges bit for bit around a sentinel; scale with factors that round; bn_fold; the Optimizer class's slot start values
and [optimizer_*] overrides; and three training steps of a session per optimizer, clip and learning-rate decay included.

The bounds are derived in optim_cases.py and are per element; tests/test_optim_cases_cpu.py shows that the f32 oracle fits them and that ten
planted faults do not.  Every test prints its worst |err| / bound per output (pytest -s)."""
import configparser

import numpy as np
import pytest
import torch

import optim_cases as O
from test_kernels_gpu import dev, host

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN = float('nan')


@pytest.fixture(scope='module')
def ops():
    from yolo_tf_amd import ops as _ops
    _ops._lib.load()
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(scope='module')
def basedir():
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        yield d


def launch(ops, kind, hp, bufs, g, n, gs, lr, alpha):
    """One optimizer entry point on device tensors bufs = (w, slots...)."""
    w, s = bufs[0], bufs[1:]
    if kind == 'adam':
        ops.adam(w, g, s[0], s[1], n, alpha, hp['beta1'], hp['beta2'], hp['epsilon'], gs)
    elif kind == 'momentum':
        ops.momentum(w, g, s[0], n, lr, hp['momentum'], gs)
    elif kind == 'gd':
        ops.sgd(w, g, n, lr, gs)
    elif kind == 'rmsprop':
        ops.rmsprop(w, g, s[0], s[1], n, lr, hp['decay'], hp['momentum'], hp['epsilon'], gs)
    elif kind == 'adagrad':
        ops.adagrad(w, g, s[0], n, lr, gs)
    elif kind == 'adadelta':
        ops.adadelta(w, g, s[0], s[1], n, lr, hp['rho'], hp['epsilon'], gs)
    else:
        ops.ftrl(w, g, s[0], s[1], n, lr, hp['learning_rate_power'], hp['l1_regularization_strength'], hp['l2_regularization_strength'], gs)


def place(a, offset):
    """The array on the device, `offset` elements behind a 16-byte aligned address; the elements around it hold NaN."""
    base = torch.full((len(a) + 8,), NAN, dtype=torch.float32, device='cuda')
    assert base.data_ptr() % 16 == 0
    t = base[offset:offset + len(a)]
    t.copy_(torch.from_numpy(np.ascontiguousarray(a, f32)))
    return base, t


def device_stepper(ops, offsets=None, differs=None):
    """optim_cases.run_chain's stepper: upload the state, one launch, read it back.  offsets: element offset of (g, w, slots...) from 16-byte
    alignment.  differs: a list that collects, per step, how many elements are not bit-equal to the f32 oracle."""
    def stepper(kind, hp, state, g, gs, lr, alpha):
        n = len(g)
        off = offsets or (0,) * (1 + len(state))
        gbase, gt = place(g, off[0])
        placed = [place(x, o) for x, o in zip(state, off[1:])]
        launch(ops, kind, hp, [t for _, t in placed], gt, n, gs, lr, alpha)
        torch.cuda.synchronize()
        for (base, t), o in zip(placed + [(gbase, gt)], tuple(off[1:]) + (off[0],)):
            edge = torch.cat([base[:o], base[o + n:]])
            assert torch.isnan(edge).all(), 'written outside the %d elements' % n
        assert np.array_equal(host(gt).view(np.uint32), np.asarray(g, f32).view(np.uint32)), 'the gradient was modified'
        new = tuple(host(t) for _, t in placed)
        if differs is not None:
            want = O.step(kind, hp, state, g, gs, f32, lr=lr, alpha=alpha)
            differs.append(sum(int((a.view(np.uint32) != np.asarray(b, f32).view(np.uint32)).sum()) for a, b in zip(new, want)))
        return new
    return stepper


def verdict(what, worst):
    print('%s: worst |err| / bound  %s' % (what, '  '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    bad = {k: v for k, v in worst.items() if k != 'decision_distance' and not v <= 1}
    assert not bad, (what, bad)
    assert worst.get('decision_distance', np.inf) >= 2, (what, worst)


def merge(total, worst):
    for k, v in worst.items():
        total[k] = min(total.get(k, np.inf), v) if k == 'decision_distance' else max(total.get(k, 0.0), v)


# ------------------------------------------------------------------------------------------------------------------
# the optimizers, step by step
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(O.CONFIGS))
def test_optimizer_steps_vs_float64_oracle(ops, name):
    """T steps at every size and gradient scale; each step against the oracle on the device's own state before it."""
    total, differs = {}, []
    for n in O.SIZES:
        for gs in O.GSCALES:
            merge(total, O.run_chain(name, n, gs, device_stepper(ops, differs=differs)))
    print('%s: %d of %d launches are not bit-equal to the f32 oracle (%d elements)' % (name, sum(d > 0 for d in differs), len(differs), sum(differs)))
    verdict(name, total)
    if name == 'adam':      # contraction is off in adam_one, divide and square root are correctly rounded: the kernel IS the f32 oracle
        assert sum(differs) == 0


@pytest.mark.parametrize('which,offsets', [('all_four_arrays_offset_by_one', (1, 1, 1, 1)), ('only_g_offset', (1, 0, 0, 0)),
                                           ('only_v_offset_by_three', (0, 0, 0, 3))])
def test_adam_scalar_path(ops, which, offsets):
    """adam_kernel takes 16-byte accesses only when all four pointers are 16-byte aligned; otherwise the scalar loop does everything."""
    total, differs = {}, []
    for n in (1, 5, 1025, 10007):
        merge(total, O.run_chain('adam', n, 1.0 / 3, device_stepper(ops, offsets, differs)))
    verdict('adam scalar path, ' + which, total)
    assert sum(differs) == 0          # the scalar and the vector path share adam_one


def test_adam_strided_loop(ops):
    """n = 2 * 8192 * 256 * 4 + 5: every thread of the largest grid takes two 16-byte groups, and the scalar tail has one element."""
    differs = []
    worst = O.run_chain('adam', O.STRIDED, 1.0 / 3, device_stepper(ops, differs=differs), steps=2)
    verdict('adam strided loop', worst)
    assert sum(differs) == 0


def test_adam_slices_that_are_no_multiple_of_4_equal_the_whole_arena_update(ops):
    """Optimizer.apply(lo, hi) with cuts at 4097 and 20003: the slices start off 16-byte alignment and take the scalar path; three steps are
    bit-identical to the whole-arena update."""
    from yolo_tf_amd.optim import Optimizer
    n = 10007 * 4
    rng = np.random.RandomState(0)
    p0 = rng.randn(n).astype(f32)
    outs = []
    for cuts in ([0, n], [0, 4097, 20003, n]):
        opt = Optimizer('adam', None, n, torch.device('cuda'))
        p = dev(p0.copy())
        assert all(t.data_ptr() % 16 == 0 for t in [p] + opt.slots)
        for t in (1, 2, 3):
            g = dev(O.gradient('adam', n, 0.5, t))
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                opt.apply(p, g, 1e-3, t, 0.5, lo, hi)
        torch.cuda.synchronize()
        outs.append([host(p)] + [host(s) for s in opt.slots])
    for a, b in zip(*outs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------
# clip_by_norm, clip_by_norm_fixed
# ------------------------------------------------------------------------------------------------------------------
CLIP_IDS = {'nseg1': 'nseg1_clipped', 'full_table': 'full_table_early_return_zero_empty_overflow_segments', 'non_finite': 'non_finite_inf_and_nan'}


@pytest.mark.parametrize('form', ['atomic', 'fixed'])
@pytest.mark.parametrize('name', list(O.CLIP_CASES), ids=[CLIP_IDS[k] for k in O.CLIP_CASES])
def test_clip_by_norm_vs_float64_oracle(ops, name, form):
    """Both forms on the same offsets table, twice on the same workspace (garbage in it before the first call: the atomic form clears its
    sums itself, the fixed form overwrites every partial)."""
    c = O.clip_case(name)
    g = dev(np.concatenate([c['g'], np.full(64, np.nan, f32)]))         # NaN behind the last segment: nobody reads or writes it
    off = torch.from_numpy(c['seg_off']).cuda()
    if form == 'atomic':
        ws = torch.full((ops.workspace_bytes('clip', c['nseg']) // 8,), 1e300, dtype=torch.float64, device='cuda')
        run = lambda: ops.clip_by_norm(g, off, c['nseg'], O.CLIP, ws)
    else:
        ws = torch.full((ops.workspace_bytes('clip_fixed', c['nseg']) // 8,), NAN, dtype=torch.float64, device='cuda')
        run = lambda: ops.clip_by_norm_fixed(g, off, c['nseg'], O.CLIP, ws)
    before = c['g']
    for call in (1, 2):
        given = before
        run()
        torch.cuda.synchronize()
        got = host(g)
        assert np.isnan(got[len(before):]).all() and np.array_equal(off.cpu().numpy(), c['seg_off'])
        worst, bad = O.clip_check(got[:len(before)], before, c['seg_off'], O.CLIP)
        print('clip_by_norm%s %s, call %d: worst |err| / (5 u |ref|) = %.3f' % ('_fixed' if form == 'fixed' else '', name, call, worst))
        assert not bad, bad
        before = got[:len(before)].copy()
    if name == 'full_table':          # the sums the second call left: those of the gradient it was given, not of the garbage before
        sums = ws.cpu().numpy().reshape(c['nseg'], -1).sum(1)
        ref = np.array([(given[a:b].astype(np.float64) ** 2).sum() for a, b in zip(c['seg_off'][:-1], c['seg_off'][1:])])
        np.testing.assert_allclose(sums, ref, rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------------------------
# zero_ranges, scale, bn_fold
# ------------------------------------------------------------------------------------------------------------------

def _zero_ranges(ops, n, ranges):
    x = dev(np.full(n, O.SENTINEL, np.uint32).view(f32))
    ops.zero_ranges(x, ranges)
    torch.cuda.synchronize()
    got = host(x).view(np.uint32)
    want = O.zero_ranges_model(np.full(n, O.SENTINEL, np.uint32), ranges)
    assert np.array_equal(got, want), '%d words differ, first at %d' % ((got != want).sum(), int(np.flatnonzero(got != want)[0]))


@pytest.mark.parametrize('name', list(O.zero_ranges_cases()))
def test_zero_ranges_bit_for_bit(ops, name):
    """+0.0 in every word of every range, every bit outside unchanged (tests/test_optim_cases_cpu.py: which branch each case reaches)."""
    _zero_ranges(ops, *O.zero_ranges_cases()[name])


def test_zero_ranges_strided_body(ops):
    _zero_ranges(ops, *O.ZERO_RANGES_STRIDED)


def test_scale_is_the_f32_product(ops):
    runs = [(n, s) for n in O.SIZES for s in O.SCALE_FACTORS] + [(O.STRIDED, 1.0 / 3)]
    outs = []
    for n, s in runs:
        x = dev(O.scale_input(n))
        ops.scale(x, n, s)
        outs.append(x)
    torch.cuda.synchronize()
    for (n, s), x in zip(runs, outs):
        want = O.scale_input(n) * f32(s)
        assert np.array_equal(host(x).view(np.uint32), want.view(np.uint32)), (n, s)


@pytest.mark.parametrize('rows,C', O.BN_FOLD_SHAPES)
def test_bn_fold_vs_float64_oracle(ops, rows, C):
    case = O.bn_fold_case(rows, C)
    W = dev(case['W'])
    Wf = torch.full((rows * C + 16,), NAN, dtype=torch.float32, device='cuda')
    bias = torch.full((C + 16,), NAN, dtype=torch.float32, device='cuda')
    ops.bn_fold(W, dev(case['gamma']), dev(case['beta']), dev(case['mean']), dev(case['var']), Wf, bias, rows, C, O.BN_EPS)
    torch.cuda.synchronize()
    assert np.array_equal(host(W).view(np.uint32), case['W'].view(np.uint32)), 'W was modified'
    assert torch.isnan(Wf[rows * C:]).all() and torch.isnan(bias[C:]).all()
    rw, rb = O.bn_fold_check(host(Wf)[:rows * C], host(bias)[:C], case)
    print('bn_fold %dx%d: worst |err| / bound: Wf %.3f bias %.3f' % (rows, C, rw, rb))
    assert rw <= 1 and rb <= 1


# ------------------------------------------------------------------------------------------------------------------
# yolo_tf_amd/optim.py
# ------------------------------------------------------------------------------------------------------------------
START = {'adam': [0.0, 0.0], 'adadelta': [0.0, 0.0], 'adagrad': [0.1], 'momentum': [0.0], 'rmsprop': [1.0, 0.0], 'ftrl': [0.1, 0.0], 'gd': []}
OVERRIDES = [('adam', 'beta1', 0.8), ('adam', 'beta2', 0.99), ('adam', 'epsilon', 1e-4), ('adadelta', 'rho', 0.9), ('adadelta', 'epsilon', 1e-6),
             ('adagrad', 'initial_accumulator_value', 0.25), ('momentum', 'momentum', 0.8), ('rmsprop', 'decay', 0.8), ('rmsprop', 'momentum', 0.5),
             ('rmsprop', 'epsilon', 1e-6), ('ftrl', 'learning_rate_power', -0.6), ('ftrl', 'initial_accumulator_value', 0.25),
             ('ftrl', 'l1_regularization_strength', 0.03), ('ftrl', 'l2_regularization_strength', 0.02)]


def _config(name, key, value):
    cfg = configparser.ConfigParser()
    cfg.add_section('optimizer_' + name)
    cfg.set('optimizer_' + name, key, repr(value))
    return cfg


def test_optimizer_slot_start_values():
    """All seven names: [TF-sem] RMSProp's ms starts at ones, Adagrad's and Ftrl's accumulators at initial_accumulator_value (also when a
    config overrides it), everything else at zero."""
    from yolo_tf_amd.optim import Optimizer, DEFAULTS
    assert set(DEFAULTS) == set(START)
    n = 1025
    for name, start in START.items():
        opt = Optimizer(name, None, n, torch.device('cuda'))
        assert len(opt.slots) == len(start), name
        for slot, value in zip(opt.slots, start):
            assert slot.dtype == torch.float32 and slot.numel() == n and np.array_equal(host(slot), np.full(n, value, f32)), (name, value)
    for name in ('adagrad', 'ftrl'):
        opt = Optimizer(name, _config(name, 'initial_accumulator_value', 0.25), n, torch.device('cuda'))
        assert np.array_equal(host(opt.slots[0]), np.full(n, 0.25, f32)), name
    with pytest.raises(KeyError):
        Optimizer('nesterov', None, n, torch.device('cuda'))


def _two_steps(name, cfg, n, lr, gs):
    """Two Optimizer.apply steps from the start values -> (the final state, the hyper-parameters, per-step worst ratios)."""
    from yolo_tf_amd.optim import Optimizer
    opt = Optimizer(name, cfg, n, torch.device('cuda'))
    rng = np.random.RandomState(7)
    w = dev(rng.randn(n).astype(f32))
    worst = {}
    for t in (1, 2):
        g = (rng.randn(n) * 10.0 ** rng.uniform(-3, 0, n)).astype(f32)
        state = tuple(host(x) for x in [w] + opt.slots)
        opt.apply(w, dev(g), lr, t, gs)
        torch.cuda.synchronize()
        new = tuple(host(x) for x in [w] + opt.slots)
        r = O.check(name, opt.hp, state, g, gs, new, lr=lr, alpha=O.alpha_of(opt.hp, lr, t) if name == 'adam' else None)
        r.pop('decision_distance', None)      # (random gradients: |linear| is nowhere near l1, and the zero pattern is asserted)
        merge(worst, r)
    return new, opt.hp, worst


@pytest.mark.parametrize('name,key,value', OVERRIDES, ids=['%s-%s' % o[:2] for o in OVERRIDES])
def test_optimizer_config_overrides_reach_the_kernel(name, key, value):
    """An [optimizer_*] option from a ConfigParser: two steps equal the oracle with the overridden value and differ from the default's."""
    from yolo_tf_amd.optim import DEFAULTS
    n, lr, gs = 1025, 0.01, 0.5
    base, hp0, worst0 = _two_steps(name, None, n, lr, gs)
    got, hp, worst = _two_steps(name, _config(name, key, value), n, lr, gs)
    assert hp0 == DEFAULTS[name] and hp == dict(DEFAULTS[name], **{key: value})
    verdict('%s default' % name, worst0)
    verdict('%s %s = %r' % (name, key, value), worst)
    assert any(not np.array_equal(a, b) for a, b in zip(base, got))
    # not in a handful of elements: in most of at least one output
    frac = max(np.mean(a != b) for a, b in zip(base, got))
    assert frac > 0.5, frac


# ------------------------------------------------------------------------------------------------------------------
# a training session: clip per tensor, learning-rate decay, the optimizer
# ------------------------------------------------------------------------------------------------------------------
SESSION_CLIP = 0.2          # the 26 tensors' gradient norms lie between 0.02 and 2.6 at these steps: about a third of them clip
SESSION_RUNS = [(name, True) for name in START] + [('adam', False)]


@pytest.mark.parametrize('name,fuse', SESSION_RUNS, ids=['%s%s' % (n, '' if f else '-unfused') for n, f in SESSION_RUNS])
def test_session_chain_of_seven_optimizers(basedir, ops, name, fuse):
    """tiny, 20 classes, 96 x 96, batch 2, f32, deterministic: three steps through forward_backward() and apply_gradients() with gradient_clip and
    an [exponential_decay] section.  Before each apply the gradients, parameters and slots are read back; afterwards the parameters and slots
    must equal the oracle chain -- R.clip_by_norm per engine.seg_off, then the step with lr_fn(global_step) and t = global_step + 1 -- under
    the bounds of optim_cases.py.  The step's reference starts from the device's own clipped gradient (the fixed-order clip run on a copy: the
    session's in-place clip must leave the same bits), which is itself held to the clip's bound."""
    from test_network_gpu import make_builder
    from yolo_tf_amd.session import TrainSession
    from yolo_tf_amd.utils import data
    b, cfg = make_builder('tiny', 20, 96, True, basedir)
    if not cfg.has_section('exponential_decay'):
        cfg.add_section('exponential_decay')
    cfg.set('exponential_decay', 'decay_steps', '2')
    cfg.set('exponential_decay', 'decay_rate', '0.5')
    cfg.set('exponential_decay', 'staircase', '1')
    sess = TrainSession(b, 2, dtype='f32', optimizer=name, learning_rate=1e-3, gradient_clip=SESSION_CLIP, config=cfg, seed=4, deterministic=True)
    sess.fuse_adam_prep = fuse
    e, opt = sess.engine, sess.optimizer
    gen = torch.Generator(device='cuda').manual_seed(11)
    seg = e.seg_off.cpu().numpy()
    assert seg[0] == 0 and seg[-1] == e.n_params and len(seg) == e.n_seg + 1
    lrs, worst, worst_clip = [], {}, 0.0
    for i in range(3):
        images = torch.rand(2, 96, 96, 3, device='cuda', generator=gen) * 255
        sess.upload_labels(data.synthetic_batch(2, 20, 3, 3, seed=40 + i))
        sess.forward_backward(images)
        torch.cuda.synchronize()
        g0 = host(e.grads)
        state = tuple(host(x) for x in [e.params] + opt.slots)
        assert np.isfinite(g0).all()
        norms = np.array([np.sqrt((g0[a:c].astype(np.float64) ** 2).sum()) for a, c in zip(seg[:-1], seg[1:])])
        # some tensors clip and some do not.  (Ftrl: only at the first step.  Its linear slot starts at 0 and knows nothing of the initial weights,
        # so the first step takes every weight to about -lr g / sqrt(accum), three orders of magnitude down, as TF's ApplyFtrl does; the
        # gradients of the steps behind it are ~1e-13 and below, down to subnormal numbers, and nothing clips any more.)
        if i == 0 or name != 'ftrl':
            assert (norms > 2 * SESSION_CLIP).sum() >= 3 and ((norms > 0) & (norms < SESSION_CLIP / 2)).sum() >= 3, sorted(norms)
        copy = e.grads.clone()
        ops.clip_by_norm_fixed(copy, e.seg_off, e.n_seg, SESSION_CLIP, torch.full_like(sess.clip_ws, NAN))
        lr, t = sess.lr_fn(sess.global_step), sess.global_step + 1
        lrs.append(lr)
        sess.apply_gradients()
        torch.cuda.synchronize()
        gc = host(copy)
        assert np.array_equal(host(e.grads).view(np.uint32), gc.view(np.uint32)), 'the session clipped something else'
        wc, bad = O.clip_check(gc, g0, seg, SESSION_CLIP)
        assert not bad, bad
        worst_clip = max(worst_clip, wc)
        new = tuple(host(x) for x in [e.params] + opt.slots)
        r = O.check(name, opt.hp, state, gc, 1.0, new, lr=lr, alpha=O.alpha_of(opt.hp, lr, t) if name == 'adam' else None)
        r.pop('decision_distance', None)
        merge(worst, r)
        assert sess.global_step == t
    assert lrs == [1e-3, 1e-3, 5e-4]
    print('session %s%s: clip worst |err| / (5 u |ref|) = %.3f' % (name, '' if fuse else ' (unfused)', worst_clip))
    verdict('session %s%s' % (name, '' if fuse else ' (unfused)'), worst)
