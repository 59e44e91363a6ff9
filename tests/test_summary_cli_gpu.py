"""train.py with `[summary] histogram` and `gradients`: the run's event file holds the five scalars, one histogram per matched variable,
<var>/gradient and <var>/gradient_norm for every trainable variable; without the keys it holds scalar events only."""
import glob
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = r'.*/(weights|biases|BatchNorm/(gamma|beta))$'


def _train(tmp_path, overlays):
    cmd = [sys.executable, 'train.py', '-c', 'config.ini', 'config/yolo2/tiny-20.ini'] + overlays + \
          ['--data', 'synthetic', '-b', '2', '-s', '2', '-d', '--seed', '1', '-n', 'run0']
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, 'FAILED: %s\n--- stdout\n%s\n--- stderr\n%s' % (' '.join(cmd), r.stdout[-3000:], r.stderr[-3000:])
    (path,) = glob.glob(os.path.join(str(tmp_path), 'yolo2', 'tiny', '20', 'run0', 'events.out.tfevents.*'))
    from yolo_tf_amd.utils import events
    return events.read_events(path)


def test_event_file_with_and_without_the_summary_keys(tmp_path):
    sys.path.insert(0, ROOT)
    from bench import make_builder
    from yolo_tf_amd.utils import events
    base = tmp_path / 'local.ini'
    base.write_text('[config]\nbasedir = %s\n' % tmp_path)
    keys = tmp_path / 'summary.ini'
    keys.write_text('[summary]\nhistogram = %s\ngradients = 1\n' % PATTERN)
    graph = make_builder('tiny', 20, 416, True, tempfile.mkdtemp(prefix='summary_cli_'))[0].graph
    trainable = {v.name: v.size for v in graph.trainable()}
    matched = {v.name: v.size for v in graph.variables.values() if re.match(PATTERN, v.name)}
    assert matched == trainable                       # (this pattern names exactly the trainable variables of the tiny network)

    evs = _train(tmp_path, [str(base), str(keys)])
    with_summary = [ev for ev in evs if ev['scalars'] or ev['histograms']]
    assert with_summary and with_summary[-1]['step'] == 2
    last = with_summary[-1]
    scalar_events = [ev for ev in evs if [t for t, _ in ev['scalars']] == list(events.SCALAR_TAGS)]
    assert scalar_events and scalar_events[-1]['step'] == 2 and not scalar_events[-1]['histograms']
    histos = dict(last['histograms'])
    assert sorted(histos) == sorted(list(matched) + [n + '/gradient' for n in trainable])
    for name, size in matched.items():
        h = histos[name]
        assert h['num'] == size and sum(h['bucket']) == size and len(h['bucket']) == len(h['bucket_limit']), name
        assert h['min'] <= h['max'] and np.all(np.diff(h['bucket_limit']) > 0), name
        assert histos[name + '/gradient']['num'] == size, name
    norms = dict(last['scalars'])
    assert sorted(norms) == sorted(n + '/gradient_norm' for n in trainable)
    for name in trainable:
        assert abs(norms[name + '/gradient_norm'] - np.sqrt(histos[name + '/gradient']['sum_squares'])) <= 1e-6 * norms[name + '/gradient_norm'], name
    assert sum(v > 0 for v in norms.values()) >= len(norms) // 2

    evs = _train(tmp_path, [str(base)])               # the same command without the overlay: scalar events only
    assert all(not ev['histograms'] for ev in evs)
    tags = [[t for t, _ in ev['scalars']] for ev in evs if ev['scalars']]
    assert tags and all(t == list(events.SCALAR_TAGS) for t in tags)
