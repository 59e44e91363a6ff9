"""`[mi355x] ema_decay` and `--ema` as a user runs them: train with the key, evaluate and detect from the averaged weights and from the raw ones; a
checkpoint trained without the key has no averages to offer."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = 'config/yolo2/tiny-20.ini'


def run(cmd, timeout=600, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert (r.returncode == 0) == ok, 'exit %d: %s\n--- stdout\n%s\n--- stderr\n%s' % (r.returncode, ' '.join(cmd), r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout + r.stderr


def _config(tmp_path, ema):
    overlay = tmp_path / 'local.ini'
    overlay.write_text('[config]\nbasedir = %s\n' % tmp_path)
    cfg = ['-c', 'config.ini', MODEL, str(overlay)]
    if ema:
        key = tmp_path / 'ema.ini'
        key.write_text('[mi355x]\nema_decay = 0.9')
        cfg.append(str(key))
    return cfg


def test_train_with_the_key_then_eval_and_detect_from_the_averages(tmp_path):
    from PIL import Image
    cfg = _config(tmp_path, ema=True)
    out = run(['train.py'] + cfg + ['--data', 'synthetic', '-b', '2', '-s', '4', '-d', '--seed', '1', '-n', 'run0', '--level', 'info'])
    assert 'ema_decay=0.9' in out, out[-2000:]
    results = {}
    for flag in (['--ema'], []):
        path = tmp_path / ('map%d.json' % len(flag))
        out = run(['eval.py'] + cfg + ['--data', 'synthetic', '--images', '4', '-b', '4', '-t', '0.000001', '--json', str(path)] + flag)
        assert 'global_step=4' in out and 'mAP07' in out, out[-2000:]
        results[bool(flag)] = json.loads(path.read_text())
    assert results[True]['ema'] is True and results[False]['ema'] is False
    assert results[True]['global_step'] == results[False]['global_step'] == 4 and results[True]['checkpoint'] == results[False]['checkpoint']
    # A uniform grey image: four steps in, the BN moving statistics are still their initial values, and on a textured image this network's box decode
    # overflows with the raw weights just as with the averaged ones -- detect.py then raises like tf.check_numerics, as it should.
    img = tmp_path / 'img.png'
    Image.fromarray(np.full((375, 500, 3), 128, np.uint8)).save(str(img))
    out = run(['detect.py', str(img)] + cfg + ['-t', '0.000001', '--level', 'info', '--ema'])
    assert 'objects detected' in out and 'global_step=4' in out, out[-2000:]


def test_eval_from_the_averages_of_a_run_without_the_key_fails(tmp_path):
    cfg = _config(tmp_path, ema=False)
    out = run(['train.py'] + cfg + ['--data', 'synthetic', '-b', '2', '-s', '1', '-d', '--seed', '1', '-n', 'run0', '--level', 'info'])
    assert 'ema_decay' not in out, out[-2000:]
    out = run(['eval.py'] + cfg + ['--data', 'synthetic', '--images', '4', '-b', '4', '--ema'], ok=False)
    assert 'model.ckpt-1.npz' in out and '[mi355x] ema_decay' in out, out[-2000:]
