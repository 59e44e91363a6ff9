"""engine.plan_binding -- which path every layer of a binding takes -- against tests/golden/engine_plans.json, the decisions of the commit that
file's header names (scripts/record_engine_plans.py lists the rows and regenerates the file): networks x batches x sizes x dtypes x training /
inference, the deterministic mode, sync-BN, every switch on its own, the calibrator's pool setting.  No device is needed."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'scripts'))

import record_engine_plans as rec

GOLDEN = json.load(open(os.path.join(HERE, 'golden', 'engine_plans.json')))


ROWS = [(dict(zip(GOLDEN['case_fields'], c)), dict(zip(GOLDEN['option_fields'], o)), GOLDEN['plans'][p]) for c, o, p in GOLDEN['rows']]


def find(**kw):
    """-> (recorded plan, convolution names, tensor names) of one row"""
    base = rec.case(kw.pop('net'), kw.pop('batch'), kw.pop('size'), kw.pop('dtype'), kw.pop('training'), **kw)
    (plan,) = [p for c, _, p in ROWS if c == base]
    g = rec.graph_of(base)
    return plan, [op['name'] for op in g.ops if op['kind'] == 'conv'], [t.name for t in g.tensors]


def test_the_table_is_the_one_the_script_lists():
    from yolo_tf_amd.engine import Options
    assert [c for c, _, _ in ROWS] == json.loads(json.dumps(rec.cases())) and len(GOLDEN['commit']) == 40
    assert tuple(GOLDEN['case_fields']) == rec.CASE_FIELDS and tuple(GOLDEN['option_fields']) == Options._fields


def test_every_row_is_decided_as_recorded():
    bad = []
    for c, options, want in ROWS:
        opts, plan = rec.plan_of(c)
        got = json.loads(json.dumps(rec.describe(plan, rec.graph_of(c))))
        if dict(opts._asdict()) != options:
            bad.append((c, 'options', options, dict(opts._asdict())))
        assert sorted(got) == sorted(want)
        for key in want:
            if got[key] != want[key]:
                bad.append((c, key, want[key], got[key]))
    assert not bad, '%d differences, the first: %r' % (len(bad), bad[0])


def test_recorded_anchors():
    """Spot values of the recording itself, so that a regenerated file cannot drift unnoticed."""
    p, convs, tensors = find(net='darknet', batch=16, size=416, dtype='bf16', training=True)
    assert convs[:21] == ['yolo2_darknet/conv%d' % i for i in range(21)] and convs[21] == 'yolo2_darknet/conv'
    assert p['pool'] == [0, 1, 4, 7] and p['fwd_pool'] == [12] and p['first_wgrad'] == [0]
    assert len(p['bn_bwd']) == 14 and [21, 20] in p['bn_bwd'] and [10, 9] in p['bn_bwd'] and [3, 2] in p['bn_bwd']
    assert 4 not in [b for _, b in p['bn_bwd']] and 'i' not in p['path']
    assert [tensors[i] for i in p['unstored']] == ['yolo2_darknet/conv%d/leaky_relu' % i for i in (0, 1, 4, 7)]
    assert p['zero_ranges'] == [[128, 128128], [52041856, 52566144], [57287808, 57812096], [62533760, 67137632]]
    p, _, _ = find(net='darknet', batch=16, size=416, dtype='bf16', training=True, deterministic=True)
    assert p['bn_bwd'] == [] and p['zero_ranges'] == [] and p['stats'] == [] and p['first_wgrad'] == []
    p, _, _ = find(net='darknet', batch=8, size=416, dtype='bf16', training=False)
    assert p['path'][0] == 'i' and p['path'].count('f') == 17 and p['fwd_pool'] == []
    p, convs, _ = find(net='tiny', batch=2, size=96, dtype='f32', training=True)
    assert convs == ['yolo2_tiny/conv%d' % i for i in range(8)] + ['yolo2_tiny/conv']
    assert p['pool'] == [0, 1, 2, 3, 4] and p['bn_bwd'] == [[7, 6], [8, 7]] and p['zero_ranges'] == [[15764352, 15861936]]
    # the calibrator's engine: only the image layer's pool fuses, so every other batch-normalised layer folds
    p, _, _ = find(net='darknet', batch=16, size=416, dtype='bf16', training=False, pools='image')
    assert p['pool'] == [0] and p['path'].count('f') == 20


def test_options_apply_what_the_modes_impose():
    from yolo_tf_amd.engine import read_options
    o = read_options(True, env={})
    assert (o.fuse_pool and o.fold_bn and o.fuse_bn_stats and o.fold_finalize and o.fuse_first_wgrad and o.fuse_bn_bwd and o.overlap_wgrad
            and o.fuse_first == 'infer' and o.side_priority == -1 and not o.deterministic and not o.sync_bn)
    d = read_options(True, deterministic=True, env={'YOLO2_FUSE_FIRST': '1'})
    assert d.deterministic and not (d.fuse_bn_stats or d.fuse_bn_bwd or d.fuse_first_wgrad) and d.fuse_first == 'infer' and d.fold_finalize
    s = read_options(True, sync_bn=True, side_priority=0, env={})
    assert s.sync_bn and not s.fold_finalize and s.fuse_bn_stats and s.side_priority == 0
    i = read_options(False, deterministic=True, sync_bn=True, env={'YOLO2_SIDE_PRIORITY': '0', 'YOLO2_FUSE_FIRST': '1'})       # inference: neither mode exists
    assert not i.deterministic and not i.sync_bn and i.fold_finalize and i.fuse_bn_stats and i.fuse_first == '1' and i.side_priority == 0


@pytest.mark.parametrize('size,batch', [(416, 16), (96, 2)])
def test_a_layer_on_the_fused_image_filter_gradient_is_always_cleared(monkeypatch, size, batch):
    """yolo2_first_layer_wgrad_bn adds with atomics whatever yolo2_conv2d_wgrad_accumulates says of the unfused kernel (it says 'stores' under
    YOLO2_FIRST_DIRECT=0, for one): the layer's weight range is in the zero ranges exactly when the plan puts it on that kernel."""
    from yolo_tf_amd import engine, ops
    monkeypatch.setattr(ops, 'conv2d_wgrad_accumulates', lambda *a: False)
    c = rec.case('darknet', batch, size, 'bf16', True)
    g = rec.graph_of(c)
    off, n = engine.layout_params(g)[0]['yolo2_darknet/conv0/weights']
    plan = engine.plan_binding(g, batch, engine._DTYPES['bf16'], True, engine.read_options(True, env={}))
    lp = plan.layers['yolo2_darknet/conv0']
    assert lp.first_wgrad and lp.zero and plan.zero_ranges == [(off, off + (n + 3) // 4 * 4)]
    assert [name for name, p in plan.layers.items() if p.zero] == ['yolo2_darknet/conv0']
    plan = engine.plan_binding(g, batch, engine._DTYPES['bf16'], True, engine.read_options(True, env={'YOLO2_FUSE_FIRST_WGRAD': '0'}))
    assert not plan.layers['yolo2_darknet/conv0'].first_wgrad and plan.zero_ranges == [] and not any(p.zero for p in plan.layers.values())
