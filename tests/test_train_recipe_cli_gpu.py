"""The training recipe as a user runs it: train.py with --accum_steps, --weight_decay and a learning-rate schedule, the checkpoint it
writes at an update boundary, and a combination it refuses."""
import configparser
import os
import re
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


def _config(tmp_path, extra=''):
    overlay = tmp_path / 'local.ini'
    overlay.write_text('[config]\nbasedir = %s\n%s' % (tmp_path, extra))
    return ['-c', 'config.ini', MODEL, str(overlay)]


def test_train_with_the_recipe_then_detect_from_its_checkpoint(tmp_path):
    from PIL import Image
    from yolo_tf_amd.optim import learning_rate_fn
    cfg = _config(tmp_path)
    out = run(['train.py'] + cfg + ['--data', 'synthetic', '-b', '2', '-s', '2', '--accum_steps', '2', '--weight_decay', '5e-4', '--lr_policy', 'steps',
                                    '--lr_steps', '1', '--lr_scales', '0.1', '--burn_in', '2', '-d', '--seed', '1', '-n', 'run0', '--level', 'info'])
    assert 'effective batch 4 (batch 2 x accum_steps 2 x world 1)' in out and 'weight_decay=0.0005 (l2)' in out, out[-3000:]
    # the two updates' learning rates, as tests/test_lr_schedule_cpu.py predicts them (train.py's default -lr is 1e-6)
    keys = configparser.ConfigParser()
    keys.read_string('[mi355x]\nlr_policy = steps\nlr_steps = 1\nlr_scales = 0.1\nburn_in = 2\n')
    want = learning_rate_fn(keys, 1e-6)
    assert want(0) == 1e-6 * 0.5 ** 4.0 and want(1) == 1e-6 * 0.1
    rates = re.findall(r'update (\d+): learning_rate=(\S+)', out)
    assert [(int(u), float(v)) for u, v in rates] == [(0, want(0)), (1, want(1))], rates
    assert 'model.ckpt-2' in out and 'model.ckpt-1' not in out and 'total_loss=' in out and 'total_loss=nan' not in out, out[-3000:]
    # (a uniform grey image: two updates in, the BN moving statistics are still near their initial values -- see tests/test_ema_cli_gpu.py)
    img = tmp_path / 'img.png'
    Image.fromarray(np.full((375, 500, 3), 128, np.uint8)).save(str(img))
    out = run(['detect.py', str(img)] + cfg + ['-t', '0.000001', '--level', 'info'])
    assert 'objects detected' in out and 'global_step=2' in out, out[-2000:]


def test_bad_combinations_exit_naming_the_key(tmp_path):
    cfg = _config(tmp_path, '[mi355x]\nshard_optimizer = true\n')
    out = run(['train.py'] + cfg + ['--data', 'synthetic', '-b', '2', '-s', '1', '--accum_steps', '2', '-d', '-n', 'run0'], ok=False)
    assert 'shard_optimizer' in out and 'accum_steps' in out and 'model.ckpt' not in out, out[-2000:]
    cfg = _config(tmp_path)
    out = run(['train.py'] + cfg + ['--data', 'synthetic', '-b', '2', '--lr_policy', 'cosine', '-d', '-n', 'run0'], ok=False)          # no -s, no lr_max_steps
    assert 'lr_max_steps' in out, out[-2000:]
    out = run(['train.py'] + cfg + ['--data', 'synthetic', '-b', '2', '-s', '1', '-o', 'ftrl', '--weight_decay', '5e-4', '--weight_decay_mode', 'decoupled', '-d', '-n', 'run0'], ok=False)
    assert 'weight_decay_mode = decoupled' in out and 'ftrl' in out, out[-2000:]
