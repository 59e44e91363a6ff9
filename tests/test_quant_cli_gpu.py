"""The int8 path as a user runs it: train a few steps, calibrate the checkpoint with quantize.py, evaluate it with eval.py in int8 and bf16."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cmd, timeout=600, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    if ok:
        assert r.returncode == 0, 'FAILED: %s\n--- stdout\n%s\n--- stderr\n%s' % (' '.join(cmd), r.stdout[-3000:], r.stderr[-3000:])
    return r.returncode, r.stdout + r.stderr


@pytest.mark.timeout_s(900)
def test_train_quantize_then_eval_in_int8_and_bf16(tmp_path):
    overlay = tmp_path / 'local.ini'
    overlay.write_text('[config]\nbasedir = %s\n' % tmp_path)
    cfg = ['-c', 'config.ini', 'config/yolo2/darknet-20.ini', str(overlay)]
    run(['train.py'] + cfg + ['--data', 'synthetic', '-b', '2', '-s', '20', '-d', '--seed', '1', '-n', 'run0', '--level', 'info'], timeout=300)
    ev = ['eval.py'] + cfg + ['--data', 'synthetic', '--images', '6', '-b', '4', '-t', '0.000001', '--mode', 'all']
    # no calibration yet: a clear error, not a traceback into the engine
    rc, out = run(ev + ['--dtype', 'int8'], timeout=120, ok=False)
    assert rc != 0 and 'no calibration file' in out and 'quantize.py' in out, out[-2000:]
    _, out = run(['quantize.py'] + cfg + ['--data', 'synthetic', '--batches', '2', '-b', '4'], timeout=180)
    assert 'global_step=20' in out and 'calibration.npz' in out, out[-2000:]
    results = {}
    for dtype in ('int8', 'bf16'):
        path = tmp_path / ('map_%s.json' % dtype)
        _, out = run(ev + ['--dtype', dtype, '--json', str(path)], timeout=240)
        assert 'global_step=20' in out and 'mAP07' in out, out[-2000:]
        results[dtype] = json.loads(path.read_text())
        assert results[dtype]['global_step'] == 20 and results[dtype]['config']['dtype'] == dtype and results[dtype]['detections'] > 0
    cal = results['int8']['calibration']
    assert cal and os.path.isfile(cal) and os.path.dirname(cal) == os.path.dirname(results['int8']['checkpoint'])
    assert results['bf16']['calibration'] is None
    # recorded, not compared: the mAP of a 20-step synthetic model is noise
    print('mAP07 int8 %r bf16 %r; mAP12 int8 %r bf16 %r' % (results['int8']['mAP07'], results['bf16']['mAP07'], results['int8']['mAP12'],
                                                            results['bf16']['mAP12']))
