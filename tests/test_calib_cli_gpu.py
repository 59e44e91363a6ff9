"""The calibration methods as a user runs them: train a few steps, calibrate the checkpoint with quantize.py --method mse, evaluate it with
eval.py in int8 from the file that wrote."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cmd, timeout=300):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, 'FAILED: %s\n--- stdout\n%s\n--- stderr\n%s' % (' '.join(cmd), r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout + r.stderr


@pytest.mark.timeout_s(600)
def test_quantize_with_a_method_then_eval_in_int8(tmp_path):
    from yolo_tf_amd import quant
    overlay = tmp_path / 'local.ini'
    overlay.write_text('[config]\nbasedir = %s\n' % tmp_path)
    cfg = ['-c', 'config.ini', 'config/yolo2/tiny-20.ini', str(overlay)]
    run(['train.py'] + cfg + ['--data', 'synthetic', '-b', '2', '-s', '5', '-d', '--seed', '1', '-n', 'run0', '--level', 'info'])
    files = {m: str(tmp_path / ('calibration_%s.npz' % m)) for m in ('absmax', 'mse')}
    q = ['quantize.py'] + cfg + ['--data', 'synthetic', '--batches', '2', '-b', '4']
    out = run(q + ['-o', files['absmax']])
    assert 'global_step=5' in out and 'threshold' not in out
    out = run(q + ['--method', 'mse', '-o', files['mse']])
    assert 'global_step=5' in out and files['mse'] in out, out[-2000:]
    base, cal = quant.Calibration.load(files['absmax']), quant.Calibration.load(files['mse'])
    assert sorted(np.load(files['absmax']).files) == ['names', 'scales'] and base.method == 'absmax'
    assert cal.method == 'mse' and set(cal.scales) == set(base.scales) == set(cal.thresholds)
    # the second pass saw the batches of the first: same abs-max, thresholds at or below it, one report line per scale class
    assert all(quant.scale_of(cal.amax[n]) == base.scales[n] for n in base.scales)
    assert all(cal.thresholds[n] <= cal.amax[n] for n in cal.scales) and any(cal.thresholds[n] < cal.amax[n] for n in cal.scales)
    lines = [line for line in out.splitlines() if 'mse threshold' in line and 'SQNR estimate' in line]
    assert sorted(n for line in lines for n in line.split(': abs-max')[0].split()) == sorted(cal.scales)
    assert 'lay above the abs-max' not in out
    path = tmp_path / 'map_int8.json'
    out = run(['eval.py'] + cfg + ['--data', 'synthetic', '--images', '6', '-b', '4', '-t', '0.000001', '--mode', 'all', '--dtype', 'int8',
                                  '--calibration', files['mse'], '--json', str(path)])
    result = json.loads(path.read_text())
    assert 'global_step=5' in out and result['config']['dtype'] == 'int8' and result['calibration'] == files['mse'] and result['detections'] > 0
