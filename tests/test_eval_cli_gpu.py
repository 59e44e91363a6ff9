"""eval.py as a user runs it: train a few steps, then evaluate the checkpoint the training run left in the logdir."""
import json
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cmd, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, 'FAILED: %s\n--- stdout\n%s\n--- stderr\n%s' % (' '.join(cmd), r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout + r.stderr


@pytest.mark.timeout_s(900)
@pytest.mark.parametrize('model_ini,mode', [('config/yolo2/darknet-20.ini', 'all'), ('config/yolo/tiny-20.ini', 'detect')])
def test_train_then_eval_from_the_logdir(tmp_path, model_ini, mode):
    overlay = tmp_path / 'local.ini'
    overlay.write_text('[config]\nbasedir = %s\n' % tmp_path)
    cfg = ['-c', 'config.ini', model_ini, str(overlay)]
    run(['train.py'] + cfg + ['--data', 'synthetic', '-b', '2', '-s', '3', '-d', '--seed', '1', '-n', 'run0', '--level', 'info'])
    out_json = tmp_path / 'map.json'
    out = run(['eval.py'] + cfg + ['--data', 'synthetic', '--images', '6', '-b', '4', '-t', '0.000001', '--mode', mode, '--json', str(out_json)])
    assert 'global_step=3' in out and 'mAP07' in out and 'mAP12' in out and 'aeroplane' in out, out[-2000:]
    r = json.loads(out_json.read_text())
    for k in ('ap07', 'ap12', 'npos', 'tp', 'fp', 'ignored', 'mAP07', 'mAP12', 'detections', 'checkpoint', 'global_step', 'config', 'names'):
        assert k in r, k
    assert r['global_step'] == 3 and os.path.exists(r['checkpoint']) and r['config']['mode'] == mode and r['images'] == 6
    assert len(r['ap07']) == len(r['ap12']) == len(r['npos']) == 20
    for a07, a12, n in zip(r['ap07'], r['ap12'], r['npos']):
        assert (math.isnan(a07) and math.isnan(a12)) if n == 0 else (0.0 <= a07 <= 1.0 and 0.0 <= a12 <= 1.0)
    assert sum(r['npos']) > 0
    if 'yolo2' in model_ini:      # YOLOv2 scores are sigmoid x softmax, 1/20 on average over the classes: some exceed 1e-6.  YOLO v1's are products of raw
        assert r['detections'] > 0      # linear outputs, which three training steps may leave at or below zero everywhere
