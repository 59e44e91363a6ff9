"""The engine launches what it launched at the commit tests/golden/engine_launches.json.gz names: the first training step and the first detection
of darknet-20 and tiny-20 at 96x96, batch 2, bf16 and f32, as tests/engine_launch_log.py records them -- every ops call that is handed a device
buffer, with its scalars, tensor dtypes and sizes and its stream.  96 is the smallest size with an even 26 -> 13-style passthrough grid; the
launch rules that depend on the batch stay covered at full size by test_network_gpu.py::test_no_layer_falls_back_to_separate_finalisation."""
import json
import os

import pytest

import engine_launch_log as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden(golden_dir):
    doc = L.read(os.path.join(golden_dir, 'engine_launches.json.gz'))
    assert (doc['batch'], doc['size']) == (L.BATCH, L.SIZE)
    return doc['logs']


@pytest.mark.parametrize('net,dtype', L.SCENARIOS)
def test_training_step_and_detection_launch_the_recorded_calls(golden, net, dtype):
    got = L.record(net, dtype)
    for phase in ('train', 'infer'):
        want, have = golden['%s %s %s' % (net, dtype, phase)], got[phase]
        assert len(want) > 20
        for i, (w, h) in enumerate(zip(want, have)):
            assert h == w, '%s %s %s: call %d differs\n recorded %s\n launched %s' % (net, dtype, phase, i, json.dumps(w), json.dumps(h))
        assert len(have) == len(want), '%s %s %s: %d calls recorded, %d launched' % (net, dtype, phase, len(want), len(have))
