"""Records what engine.plan_binding decides for a table of networks, batches, sizes and switches: tests/golden/engine_plans.json.

    python scripts/record_engine_plans.py [--out tests/golden/engine_plans.json] [--commit NAME]

Pure host work: no device is touched (the library's host queries assume 256 compute units without one, the MI355X's count).  Run it when a
pull request changes one of the engine's decisions on purpose; tests/test_engine_plan_cpu.py reproduces every row from the plan function.
The file's header names the commit whose decisions it holds."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWITCHES = [('YOLO2_FUSE_POOL', '0'), ('YOLO2_FOLD_BN', '0'), ('YOLO2_FUSE_BN_STATS', '0'), ('YOLO2_FOLD_FINALIZE', '0'), ('YOLO2_FUSE_FIRST', '1'),
            ('YOLO2_FUSE_FIRST', '0'), ('YOLO2_FUSE_FIRST_WGRAD', '0'), ('YOLO2_FUSE_BN_BWD', '0'), ('YOLO2_OVERLAP_WGRAD', '0'), ('YOLO2_SIDE_PRIORITY', '0')]


def case(net, batch, size, dtype, training, deterministic=False, sync_bn=False, env=None, pools='all'):
    return dict(net=net, batch=batch, size=size, dtype=dtype, training=training, deterministic=deterministic, sync_bn=sync_bn, env=env or {}, pools=pools)


def cases():
    out = []
    for net in ('darknet', 'tiny'):
        for batch in (16, 8, 4, 2):
            for size in (416, 96, 320, 608):
                for dtype in ('bf16', 'f32'):
                    for training in (True, False):
                        out.append(case(net, batch, size, dtype, training))
    for batch in (16, 2):                   # YOLO (v1) tiny: the fully connected head fixes the input size
        for dtype in ('bf16', 'f32'):
            for training in (True, False):
                out.append(case('v1tiny', batch, None, dtype, training))
    for net, batch, size, dtype in (('darknet', 16, 416, 'bf16'), ('tiny', 2, 96, 'f32')):
        out.append(case(net, batch, size, dtype, True, deterministic=True))
        out.append(case(net, batch, size, dtype, True, sync_bn=True))
        for name, value in SWITCHES:
            for training in (True, False):
                out.append(case(net, batch, size, dtype, training, env={name: value}))
        out.append(case(net, batch, size, 'bf16', False, pools='image'))      # quant.Calibrator's engine
    return out


_graphs = {}


def graph_of(c):
    """The traced graph of a case (cached: the plan never changes a graph)."""
    key = (c['net'], c['size'], c['training'])
    if key not in _graphs:
        from yolo_tf_amd import utils
        from yolo_tf_amd.model import yolo, yolo2
        family, ini = ('yolo', 'tiny-20.ini') if c['net'] == 'v1tiny' else ('yolo2', '%s-20.ini' % c['net'])
        cfg = utils.make_config([os.path.join(ROOT, 'config.ini'), os.path.join(ROOT, 'config', family, ini)], tempfile.mkdtemp(prefix='engine_plans_'))
        cfg.set('cache', 'names', os.path.join(ROOT, cfg.get('cache', 'names')))
        if family == 'yolo2':
            cfg.set('yolo2', 'anchors', os.path.join(ROOT, cfg.get('yolo2', 'anchors')))
            cfg.set('yolo2', 'width', str(c['size']))
            cfg.set('yolo2', 'height', str(c['size']))
        utils.ensure_names(cfg)
        b = (yolo if family == 'yolo' else yolo2).Builder(None, cfg)
        b(None, training=c['training'])
        _graphs[key] = b.graph
    return _graphs[key]


CASE_FIELDS = ('net', 'batch', 'size', 'dtype', 'training', 'deterministic', 'sync_bn', 'env', 'pools')
PATHS = {'fold': 'f', 'first': 'i', 'bn': 'b', 'bias_leaky': 'l', 'bias': 'p'}


def describe(plan, graph):
    """One binding's decisions as compact JSON-ready data: a convolution is its position among the graph's convolutions, a tensor its position
    in graph.tensors.  path: one letter per convolution (PATHS); fin: the *_fin row limit per convolution; bn_bwd: [consumer, producer] pairs."""
    L = list(plan.layers.values())
    conv = {n: i for i, n in enumerate(plan.layers)}
    tensor = {t: i for i, t in enumerate(graph.tensors)}
    return dict(path=''.join(PATHS[p.path] for p in L),
                pool=[i for i, p in enumerate(L) if p.pool is not None],
                fwd_pool=[i for i, p in enumerate(L) if p.fwd_pool is not None],
                stats=[i for i, p in enumerate(L) if p.stats],
                fin=[p.fin_limit for p in L],
                first_wgrad=[i for i, p in enumerate(L) if p.first_wgrad],
                bn_bwd=[[i, conv[p.bn_bwd['name']]] for i, p in enumerate(L) if p.bn_bwd is not None],
                zero=[i for i, p in enumerate(L) if p.zero],
                zero_ranges=[list(r) for r in plan.zero_ranges],
                unstored=sorted(tensor[t] for t in plan.unstored))


def plan_of(c):
    from yolo_tf_amd import engine
    opts = engine.read_options(c['training'], c['deterministic'], c['sync_bn'], env=c['env'])
    return opts, engine.plan_binding(graph_of(c), c['batch'], engine._DTYPES[c['dtype']], c['training'], opts, c['pools'])


def write(path, commit, rows):
    """rows: [(case, Options as a dict, described plan)].  Equal plans are stored once; a row is [case values, option values, plan index]."""
    from yolo_tf_amd.engine import Options
    plans, keys, out = [], {}, []
    for c, o, p in rows:
        key = json.dumps(p, sort_keys=True, separators=(',', ':'))
        if key not in keys:
            keys[key] = len(plans)
            plans.append(key)
        out.append(json.dumps([[c[f] for f in CASE_FIELDS], [o[f] for f in Options._fields], keys[key]], separators=(',', ':')))
    with open(path, 'w') as f:
        f.write('{\n "commit": %s,\n "case_fields": %s,\n "option_fields": %s,\n "plans": [\n' % (
            json.dumps(commit), json.dumps(list(CASE_FIELDS)), json.dumps(list(Options._fields))))
        f.write(',\n'.join('  ' + p for p in plans))
        f.write('\n ],\n "rows": [\n')
        f.write(',\n'.join('  ' + r for r in out))
        f.write('\n ]\n}\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'engine_plans.json'))
    ap.add_argument('--commit', default=None, help='the commit whose decisions these are (default: the checkout\'s HEAD)')
    args = ap.parse_args()
    commit = args.commit or subprocess.run(['git', '-C', ROOT, 'rev-parse', 'HEAD'], capture_output=True, text=True).stdout.strip() or 'unknown'
    rows = []
    for c in cases():
        opts, plan = plan_of(c)
        rows.append((c, dict(opts._asdict()), describe(plan, graph_of(c))))
    write(args.out, commit, rows)
    print('wrote %s: %d rows' % (args.out, len(rows)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
