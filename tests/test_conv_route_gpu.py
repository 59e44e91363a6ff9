"""The launch does what the route says, and computes what the library computed before the rule became a pure function.

Every default-environment row of tests/golden/conv_plans.json (scripts/record_conv_plans.py) is launched once more: yolo2_debug_last_conv_plan,
yolo2_last_bn_part_rows and *pending have to equal ops.conv_route at the device's own CU count, and -- for the rows recorded on seeded operands --
yolo2_crc32c of the output buffer has to equal the recorded checksum (same kernel, same launch parameters, same bytes).  One launch per row."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'scripts'))
GOLDEN = json.load(open(os.path.join(HERE, 'golden', 'conv_plans.json')))
MODE = {'conv2d': 'plain', 'ws': 'plain', 'conv2d_bias': 'bias_act', 'ws_bias': 'bias_act', 'bias_leaky': 'bias_act', 'bn': 'bn', 'dgrad_bn': 'dgrad_bn'}


def test_default_rows_launch_what_the_route_names_and_store_the_recorded_bytes():
    import record_conv_plans as rec
    from yolo_tf_amd import ops
    ops._lib.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = [r for r in GOLDEN['rows'] if not r['env']]
    assert len(rows) > 300
    spec = [{k: r[k] for k in ('entry', 'dtype', 'B', 'H', 'W', 'Cp', 'ldp', 'Nf', 'ldo', 'k', 'ws_floats', 'det', 'wgs', 'tag')} for r in rows]
    assert [r['index'] for r in rows] == list(range(len(rows)))      # (the seed of a row's operands is its index)
    got, _ = rec.run_rows(spec, 0)
    bad, checked = [], 0
    for r, g in zip(rows, got):
        dtype = torch.bfloat16 if r['dtype'] == 'bf16' else torch.float32
        ops.set_deterministic(r['det'])
        try:
            route = ops.conv_route(r['B'], r['H'], r['W'], r['Cp'], r['ldp'], r['Nf'], r['ldo'], r['k'], dtype, MODE[r['entry']], 4 * r['ws_floats'], cus=r['wgs'] or cus)
        finally:
            ops.set_deterministic(0)
        plan = [route['plan'][k] for k in ops.CONV_PLAN_KEYS]
        if g['plan'] != plan or (g['rows'] is not None and g['rows'] != route['rows']) or (g['pending'] or 0) != route['pending']:
            bad.append(('route', r['index'], r['tag'], g['plan'], g['rows'], g['pending'], route))
        if r['crc'] is not None and cus == GOLDEN['cus']:      # (another CU count: other grids, other summation orders)
            checked += 1
            if g['crc'] != r['crc']:
                bad.append(('crc', r['index'], r['tag'], r['entry'], r['dtype'], r['plan'], g['plan'], r['crc'], g['crc']))
    assert not bad, '%d rows differ, the first: %s' % (len(bad), bad[:4])
    assert cus != GOLDEN['cus'] or checked > 150
