"""HistogramSummaries over a real training step: every variable, batch moment, stored activation and gradient of the tiny network, binned on the
device, equals the specification (tests/summary_ref.py) applied to host copies of the same tensors."""
import math
import os
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import summary_ref as S  # noqa: E402
from test_summary_cpu import _config  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('dtype,deterministic', [('bf16', False), ('f32', False), ('bf16', True)])
def test_summaries_of_one_step_match_the_specification(dtype, deterministic):
    import torch
    sys.path.insert(0, ROOT)
    from bench import make_builder
    from yolo_tf_amd.session import TrainSession
    from yolo_tf_amd.summary import HistogramSummaries, activation_tag
    from yolo_tf_amd.utils import data
    B, size = 2, 96
    b, _ = make_builder('tiny', 20, size, True, tempfile.mkdtemp(prefix='summary_engine_'))
    sess = TrainSession(b, B, dtype=dtype, optimizer='adam', learning_rate=1e-3, seed=3, deterministic=deterministic)
    e = sess.engine
    images = torch.rand(B, size, size, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(0)) * 255
    sess.step(images, data.synthetic_batch(B, 20, size // 32, size // 32, seed=1))
    hs = HistogramSummaries(sess, _config('.*', gradients=1))
    hs.collect()
    histograms, scalars = hs.results()
    got = dict(histograms)
    assert len(got) == len(histograms)                      # no tag twice
    # what the specification says about host copies of the same tensors
    want = {}
    variables, gradients = e.get_variables(), e.get_gradients()
    for name, v in variables.items():
        want[name] = v
    for name, g in gradients.items():
        want[name + '/gradient'] = g
    for op in e.graph.ops:
        if op['kind'] == 'conv' and op['bn']:
            want[op['name'] + '/BatchNorm/moments/normalize/mean'] = e.conv[op['name']]['mean'].cpu().numpy()
            want[op['name'] + '/BatchNorm/moments/normalize/variance'] = e.conv[op['name']]['var'].cpu().numpy()
    inputs = set(e.graph.inputs.values())
    stored = skipped = 0
    for t, where in e.summarizable_tensors():
        tag = activation_tag(t.name, 'yolo2_tiny', t in inputs)
        if where is None:
            skipped += 1
            assert tag not in got
            continue
        buf, rows, c, ld = where
        a = buf[:(rows - 1) * ld + c].float().cpu().numpy()
        a = np.concatenate([a, np.zeros(ld - c, a.dtype)]).reshape(rows, ld)[:, :c]         # padding stripped
        assert a.shape == (B * t.h * t.w, t.c)
        want[tag] = a
        stored += 1
    assert stored >= 10 and skipped >= 1                    # the layers fused with their max pool never store their activation
    assert 'yolo2_tiny/input' in want and 'yolo2_tiny/conv0/convolution' in want and 'yolo2_tiny/conv7/leaky_relu/data' in want
    assert sorted(got) == sorted(want)
    for tag, values in want.items():
        ref, g = S.histogram(values), got[tag]
        assert g['nonfinite'] == 0 and g['num'] == ref['num'] == np.asarray(values).size, tag
        assert np.array_equal(g['counts'], ref['counts']), (tag, np.nonzero(g['counts'] != ref['counts'])[0][:8])
        assert g['min'] == ref['min'] and g['max'] == ref['max'], tag
        bs, bq = S.sum_bounds(ref)
        assert abs(g['sum'] - ref['sum']) <= bs and abs(g['sum_squares'] - ref['sum_squares']) <= bq, tag
    # gradient norms: one per trainable variable, NumPy's to 1e-12
    norms = dict(scalars)
    assert sorted(norms) == sorted(n + '/gradient_norm' for n in gradients)
    some = 0
    for name, g in gradients.items():
        ref = math.sqrt(float(np.sum(g.astype(np.float64) ** 2)))
        assert abs(norms[name + '/gradient_norm'] - ref) <= 1e-12 * ref, (name, norms[name + '/gradient_norm'], ref)
        some += ref > 0
    assert some >= len(gradients) // 2
    # a second collection of the unchanged state: the same bytes
    hs.collect()
    again, _ = hs.results()
    for (t1, r1), (t2, r2) in zip(histograms, again):
        assert t1 == t2 and np.array_equal(r1['counts'], r2['counts']) and all(r1[k] == r2[k] for k in ('min', 'max', 'sum', 'sum_squares', 'num'))
