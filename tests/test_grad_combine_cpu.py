"""The NumPy specification of yolo2_grad_combine (tests/grad_combine_ref.py) against a float64 restatement, and the table of decayed ranges a TrainSession
builds, on a traced `tiny` graph.  No GPU.

The bound.  With u = 2^-24 (f32 round to nearest) and the f32 values of scale and decay taken as exact numbers, mode FINAL computes
    s1 = fl(acc + g), s2 = fl(s1 * scale), t = fl(decay * w), s3 = fl(s2 + t)
against E = (acc + g) * scale + decay * w.  With A = |(acc + g) * scale| and T = |decay * w|:
    |s2 - (acc + g) * scale| <= A * ((1 + u)^2 - 1) = A * (2u + u^2),     |t - decay * w| <= T * u,
    |s3 - (s2 + t)| <= u * |s2 + t| <= u * (A * (1 + u)^2 + T * (1 + u)),
so |s3 - E| <= u * A * (3 + 3u + u^2) + u * T * (2 + u) <= u * (3 * A + 2 * T) * (1 + 2u): three roundings on the gradient's path, two on the decay term's.
Nothing underflows at the magnitudes used (the smallest product is far above 2^-126), so no absolute term is needed; one denormal ulp (2^-149) is allowed anyway.
ADD is one rounding (u * |acc + g|), the shrink one (u * |w * shrink|)."""
import numpy as np
import pytest

import grad_combine_ref as ref

U = 2.0 ** -24
N = 20011


@pytest.fixture(scope='module')
def arenas():
    rng = np.random.RandomState(3)
    return [(rng.standard_normal(N) * s).astype(np.float32) for s in (1e-2, 3e-2, 0.5)]


RANGES = [(1, 3), (5, 6), (6, 4099), (9000, N)]


@pytest.mark.parametrize('has_acc', [True, False])
@pytest.mark.parametrize('scale', [1.0, float(np.float32(1.0 / 3.0)), 1.0 / 8.0])
@pytest.mark.parametrize('decay,shrink', [(0.0, 1.0), (5e-4, 1.0), (0.0, float(np.float32(1.0 - 1e-3 * 5e-4))), (5e-4, float(np.float32(1.0 - 1e-3 * 5e-4)))])
def test_final_within_the_three_rounding_bound_of_float64(arenas, has_acc, scale, decay, shrink):
    g, acc, w = arenas
    sg, sacc, sw = ref.combine(g, acc if has_acc else None, w, ref.FINAL, scale, decay, shrink, RANGES)
    m = ref.mask(N, RANGES)
    g64, a64, w64 = g.astype(np.float64), acc.astype(np.float64) * has_acc, w.astype(np.float64)
    first = (a64 + g64) * np.float64(np.float32(scale))
    term = np.where(m, np.float64(np.float32(decay)) * w64, 0.0)
    bound = U * (3 * np.abs(first) + 2 * np.abs(term)) * (1 + 2 * U) + 2.0 ** -149
    err = np.abs(sg.astype(np.float64) - (first + term))
    assert sg.dtype == np.float32 and np.all(err <= bound), float((err / bound).max())
    if decay:
        assert np.any(term != 0) and np.any(sg[m] != ref.combine(g, acc if has_acc else None, w, ref.FINAL, scale, 0.0, 1.0, RANGES)[0][m])
    want_w = np.where(m, w64 * np.float64(np.float32(shrink)), w64)
    assert np.all(np.abs(sw.astype(np.float64) - want_w) <= U * np.abs(want_w) + 2.0 ** -149)
    assert np.array_equal(sw[~m].view(np.int32), w[~m].view(np.int32))                 # outside the ranges: w's own bits
    assert (shrink == 1.0) == np.array_equal(sw.view(np.int32), w.view(np.int32))
    assert sacc is None or np.array_equal(sacc.view(np.int32), acc.view(np.int32))
    # the inputs were not written
    assert np.array_equal(arenas[0], g) and sg is not g and sw is not w


def test_store_add_and_the_whole_accumulation(arenas):
    g, acc, w = arenas
    _, s, _ = ref.combine(g, None, None, ref.STORE)
    assert np.array_equal(s.view(np.int32), g.view(np.int32)) and s is not g
    _, a, _ = ref.combine(g, acc, None, ref.ADD)
    exact = acc.astype(np.float64) + g.astype(np.float64)
    assert a.dtype == np.float32 and np.all(np.abs(a.astype(np.float64) - exact) <= U * np.abs(exact) + 2.0 ** -149)
    # K micro-gradients: STORE, ADD, ..., FINAL with f32(1 / K); K = 1 is FINAL alone, without an accumulator
    grads = [g, acc, (g * np.float32(-0.5)).astype(np.float32)]
    out, w3 = ref.accumulate(grads, w, 5e-4, 1.0, RANGES)
    by_hand = ref.combine(grads[2], ref.combine(grads[1], ref.combine(grads[0], None, None, ref.STORE)[1], None, ref.ADD)[1], w, ref.FINAL,
                          np.float32(1.0 / 3.0), 5e-4, 1.0, RANGES)[0]
    assert np.array_equal(out.view(np.int32), by_hand.view(np.int32)) and np.array_equal(w3.view(np.int32), w.view(np.int32))
    mean = sum(x.astype(np.float64) for x in grads) / 3.0 + np.where(ref.mask(N, RANGES), 5e-4 * w.astype(np.float64), 0.0)
    assert np.allclose(out, mean, rtol=1e-5, atol=1e-8)
    one, _ = ref.accumulate([g], w, 0.0, 1.0, RANGES)
    assert np.array_equal(one.view(np.int32), ref.combine(g, None, w, ref.FINAL, 1.0)[0].view(np.int32))
    nz = g != 0
    assert np.array_equal(one[nz].view(np.int32), g[nz].view(np.int32))                # (* 1.0f is exact)


def test_specials_propagate_as_ieee_says():
    g = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-41, 1.0], np.float32)
    acc = np.array([1.0, -np.inf, -np.inf, -0.0, 1e-41, np.nan], np.float32)
    w = np.array([1.0, 1.0, 1.0, -0.0, np.inf, 1.0], np.float32)
    out, _, sw = ref.combine(g, acc, w, ref.FINAL, 0.5, 5e-4, 0.5, [(0, 6)])
    assert np.isnan(out[0]) and np.isnan(out[1]) and out[2] == -np.inf and np.isnan(out[5]) and out[4] == np.inf
    assert out[3] == 0 and np.signbit(out[3])                                           # -0 + -0 = -0, * 0.5 = -0, + (5e-4 * -0 = -0) = -0
    assert sw[4] == np.inf and np.signbit(sw[3])
    out, _, _ = ref.combine(g, acc, w, ref.FINAL, 0.5, 0.0, 1.0, [(0, 6)])               # decay == 0: no term at all, an infinite weight stays out of the gradient
    assert out[4] == np.float32(1e-41) and np.array_equal(ref.combine(g, acc, w, ref.FINAL, 0.5, 0.0, 1.0, [])[0].view(np.int32), out.view(np.int32))


def _graph(inference='tiny'):
    from yolo_tf_amd import graph as G
    from yolo_tf_amd.model.yolo2 import inference as inf
    g = G.Graph()
    x = G.placeholder(g, 'image', 96, 96)
    getattr(inf, inference)(x, 20, 5, training=True)
    return g


def test_decay_ranges_cover_the_filters_only():
    from yolo_tf_amd import ops
    from yolo_tf_amd.engine import layout_params
    from yolo_tf_amd.session import decay_ranges
    g = _graph()
    offsets, total = layout_params(g)
    ranges = decay_ranges(offsets)
    assert ranges == ref.weight_ranges(offsets) == ops.check_grad_ranges(ranges, total)        # sorted, disjoint, inside the arena
    assert all(b < e for b, e in ranges) and all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:]))
    covered = ref.mask(total, ranges)
    convs = [op for op in g.ops if op['kind'] == 'conv']
    assert len(ranges) == len(convs) >= 9
    for name, (o, n) in offsets.items():
        kind = name.rsplit('/', 1)[-1]
        assert kind in ('weights', 'gamma', 'beta', 'biases'), name
        assert covered[o:o + n].all() if kind == 'weights' else not covered[o:o + n].any(), name
    assert int(covered.sum()) == sum(offsets[op['weights'].name][1] for op in convs)                # ... and none of the padding between variables
    assert any(e % 4 for _, e in ranges) or any((e - b) % 64 for b, e in ranges)                    # a filter that ends off the arena's alignment


def test_recipe_options_and_refusals():
    import configparser
    from yolo_tf_amd.session import recipe_options, refuse_recipe
    cfg = configparser.ConfigParser()
    assert recipe_options(None) == recipe_options(cfg) == (1, 0.0, 'l2')
    cfg.read_string('[mi355x]\naccum_steps = 8\nweight_decay = 0.0005\nweight_decay_mode = Decoupled\n')
    assert recipe_options(cfg) == (8, 0.0005, 'decoupled')
    assert recipe_options(cfg, accum_steps=1, weight_decay=0.0, weight_decay_mode='l2') == (1, 0.0, 'l2')      # an argument wins over the key
    for kw, key in (({'accum_steps': 0}, 'accum_steps'), ({'accum_steps': -2}, 'accum_steps'), ({'accum_steps': '2.5'}, 'accum_steps'),
                    ({'weight_decay': -1e-4}, 'weight_decay'), ({'weight_decay': float('nan')}, 'weight_decay'), ({'weight_decay': 'x'}, 'weight_decay'),
                    ({'weight_decay_mode': 'adamw'}, 'weight_decay_mode')):
        with pytest.raises(ValueError, match=key):
            recipe_options(None, **kw)
    refuse_recipe(1, 0.0, 'l2', v1=True, shard_optimizer=True, optimizer='ftrl')                              # off: nothing to refuse
    refuse_recipe(4, 5e-4, 'decoupled', v1=False, shard_optimizer=False, optimizer='adam')
    refuse_recipe(1, 5e-4, 'l2', v1=True, shard_optimizer=False, optimizer='ftrl')
    with pytest.raises(NotImplementedError, match='accum_steps'):
        refuse_recipe(2, 0.0, 'l2', v1=True, shard_optimizer=False, optimizer='adam')
    with pytest.raises(NotImplementedError, match=r'shard_optimizer.*accum_steps'):
        refuse_recipe(2, 0.0, 'l2', v1=False, shard_optimizer=True, optimizer='adam')
    with pytest.raises(NotImplementedError, match=r'shard_optimizer.*weight_decay'):
        refuse_recipe(1, 5e-4, 'l2', v1=False, shard_optimizer=True, optimizer='adam')
    with pytest.raises(NotImplementedError, match=r'weight_decay_mode = decoupled.*ftrl'):
        refuse_recipe(1, 5e-4, 'decoupled', v1=False, shard_optimizer=False, optimizer='ftrl')
