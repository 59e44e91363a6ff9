"""The convolution launch rule, pinned without a device.

tests/golden/conv_plans.json holds, for a few hundred calls, what the library did BEFORE the rule became a pure function (recorded by launching:
scripts/record_conv_plans.py): the plan words of yolo2_debug_last_conv_plan, the partial rows, *pending, and the values of the two shape queries.
ops.conv_route (csrc/conv_route.hip y2_conv_route, the function the launch itself calls) has to reproduce every row at the recorded CU count.
Rows recorded under an environment knob are queried with the matching exclusion, or -- YOLO2_IGEMM_TAP=3 -- with the debug setter the knob initialises."""
import json
import os
import re

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, 'golden', 'conv_plans.json')))
ROWS = GOLDEN['rows']
MODE = {'conv2d': 'plain', 'ws': 'plain', 'conv2d_bias': 'bias_act', 'ws_bias': 'bias_act', 'bias_leaky': 'bias_act', 'bn': 'bn', 'dgrad_bn': 'dgrad_bn'}
EXCLUDE = {'YOLO2_C32': 'c32', 'YOLO2_C64': 'c64', 'YOLO2_D1': 'd1', 'YOLO2_FIRST_DIRECT': 'first', 'YOLO2_IGEMM_STREAM': 'stream', 'YOLO2_IGEMM_TAP': 'tap'}
# table lines no recorded row reaches: (line, reason).  At most four.
UNREACHED = []


@pytest.fixture(scope='module')
def ops():
    from yolo_tf_amd import ops as _ops
    _ops._lib.load()
    return _ops


def route_of(ops, r, cus):
    """ops.conv_route for a golden row, under the knob the row was recorded with."""
    exclude, tap = [], None
    for name, value in r['env'].items():
        if name == 'YOLO2_IGEMM_TAP' and value != '0':
            tap = int(value)
        else:
            assert value == '0', (name, value)
            exclude.append(EXCLUDE[name])
    dtype = torch.bfloat16 if r['dtype'] == 'bf16' else torch.float32
    ops.set_deterministic(r['det'])
    if tap is not None:
        ops.set_igemm_tap(tap)
    try:
        return ops.conv_route(r['B'], r['H'], r['W'], r['Cp'], r['ldp'], r['Nf'], r['ldo'], r['k'], dtype, MODE[r['entry']], 4 * r['ws_floats'],
                              cus=r['wgs'] or cus, exclude=exclude)
    finally:
        ops.set_deterministic(0)
        if tap is not None:
            ops.set_igemm_tap(2)


def expected_stats(r):
    """Where the recorded call took its statistics from, as far as the recording shows it."""
    if r['entry'] == 'dgrad_bn':
        return 'epilogue' if r['pending'] else 'two_step'
    if r['entry'] == 'bn':
        return 'colsum' if r['plan'][5] == 1 else 'epilogue'      # K-sliced grids: a pass over the finished output
    return 'none'


def test_golden_file_is_what_the_tests_assume():
    assert GOLDEN['plan_keys'] == ['BM', 'BN', 'waves', 'chunks', 'stages', 'split', 'grid_x', 'grid_y']
    assert GOLDEN['ws_floats'] == 1024 + 256 * 256 * 128 and GOLDEN['cus'] > 0 and len(ROWS) > 300
    assert {tuple(sorted(r['env'].items())) for r in ROWS} >= {(), (('YOLO2_C32', '0'),), (('YOLO2_C64', '0'),), (('YOLO2_D1', '0'),), (('YOLO2_FIRST_DIRECT', '0'),),
                                                              (('YOLO2_IGEMM_TAP', '0'),), (('YOLO2_IGEMM_TAP', '3'),), (('YOLO2_IGEMM_STREAM', '0'),)}


def test_every_golden_row_is_reproduced_by_the_route(ops):
    bad = []
    for r in ROWS:
        got = route_of(ops, r, GOLDEN['cus'])
        plan = [got['plan'][k] for k in ops.CONV_PLAN_KEYS]
        want_rows = r['rows'] if r['rows'] is not None else got['rows']      # (recorded for the statistics-producing entry points only)
        if (plan, got['rows'], got['pending'], got['stats']) != (r['plan'], want_rows, r['pending'] or 0, expected_stats(r)):
            bad.append((r['index'], r['tag'], r['entry'], r['env'], r['plan'], r['rows'], r['pending'], got))
    assert not bad, '%d of %d rows differ, the first: %s' % (len(bad), len(ROWS), bad[:3])


def test_shape_queries_equal_the_recorded_values(ops):
    from yolo_tf_amd import _lib
    for r in ROWS:
        if r['env']:
            continue
        dt = _lib.BF16 if r['dtype'] == 'bf16' else _lib.F32
        # (the workspace query sizes for the device's own CU count: 256 on a host without a device, the recorded count)
        assert int(_lib.query('yolo2_conv2d_workspace_bytes', r['B'], r['H'], r['W'], r['Cp'], r['Nf'], r['k'], dt)) == r['ws_bytes_query'], r
        assert int(_lib.query('yolo2_conv2d_dgrad_bn_fuses', r['B'], r['H'], r['W'], r['Nf'], r['k'], dt)) == r['fuses_query'], r


def test_route_query_is_pure(ops):
    before = (ops.last_conv_plan(), ops.last_bn_part_rows())
    for r in ROWS[::7]:
        a = route_of(ops, r, GOLDEN['cus'])
        assert a == route_of(ops, r, GOLDEN['cus'])
        assert (ops.last_conv_plan(), ops.last_bn_part_rows()) == before


def table_lines():
    """conv_igemm_table.h: ROW(BM, BN, WGN, stages, split, ctail, chunks, waves, kernel sizes, twins) -> every instantiation the row stands for, as
    (T, BM, BN, WGN, stages, KS, split, ctail, chunks, waves, bnbwd).  Every row is built for both dtypes; twins: the BN-backward forms."""
    text = open(os.path.join(HERE, '..', 'yolo_tf_amd', 'csrc', 'conv_igemm_table.h')).read()
    lines = []
    for m in re.finditer(r'^\s*ROW\(([\d,\s]+),\s*(K31|K3),\s*(BOTH|BF16|NONE)\)', text, re.M):
        BM, BN, WGN, stages, split, ctail, chunks, waves = [int(x) for x in m.group(1).split(',')]
        for KS in ((3, 1) if m.group(2) == 'K31' else (3,)):
            for T in ('float', 'bf16'):
                lines.append((T, BM, BN, WGN, stages, KS, split, ctail, chunks, waves, 0))
                if m.group(3) == 'BOTH' or (m.group(3) == 'BF16' and T == 'bf16'):
                    lines.append((T, BM, BN, WGN, stages, KS, split, ctail, chunks, waves, 1))
    assert len(lines) == len(set(lines)) >= 60
    return lines


def test_every_table_line_is_reached_by_a_golden_row(ops):
    """The line a route names, rebuilt from the plan words: (T, BM, BN, WGN, stages, KS, split, ctail, chunks, waves, bnbwd)."""
    reached = set()
    for r in ROWS:
        got = route_of(ops, r, GOLDEN['cus'])
        if got['family'] != 'igemm':
            continue
        p = got['plan']
        vec = 8 if r['dtype'] == 'bf16' else 4
        bnbwd = int(r['entry'] == 'dgrad_bn' and got['stats'] == 'epilogue')
        ctail = int(r['Cp'] % (4 * vec) != 0 and not bnbwd and p['chunks'] == 4)
        reached.add(('bf16' if r['dtype'] == 'bf16' else 'float', p['BM'], p['BN'], 2 if p['BN'] == 128 else 1, p['stages'], r['k'], p['split'] & 0xff, ctail,
                     p['chunks'], p['waves'], bnbwd))
    lines = set(table_lines())
    assert reached <= lines, 'routes name lines the table does not have: %s' % sorted(reached - lines)
    assert len(UNREACHED) <= 4
    assert lines - reached == {l for l, _ in UNREACHED}, sorted(lines - reached)
    assert len(lines) == 80
