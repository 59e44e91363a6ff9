"""`train.py --box_loss MODE` as a user runs it: a short run logs the mode and a finite loss; an unknown value is refused by argparse and the
YOLO (v1) family before anything is built."""
import os
import re

import numpy as np
import pytest

from test_multiscale_cli_gpu import config, run

pytestmark = pytest.mark.gpu


def test_train_with_ciou(tmp_path):
    cfg = config(tmp_path, multiscale=None)
    out = run(['train.py'] + cfg + ['--data', 'synthetic', '-b', '2', '-s', '2', '-d', '--seed', '0', '-n', 'run0', '--level', 'info', '--box_loss', 'ciou'])
    assert 'box_loss: ciou (1 - CIoU of the responsible box, weighted by [yolo2_hparam] coords = ' in out, out[-2000:]
    losses = [float(v) for v in re.findall(r'total_loss=(\S+)', out)]
    assert losses and np.all(np.isfinite(losses)), out[-2000:]
    assert 'model.ckpt-2' in out


def _with_key(tmp_path, value):
    cfg = config(tmp_path, multiscale=None)
    with open(cfg[-1], 'a') as f:
        f.write('[mi355x]\nbox_loss = %s\n' % value)
    return cfg


def test_flag_wins_over_the_config_key_in_both_directions(tmp_path):
    tail = ['--data', 'synthetic', '-b', '2', '-s', '2', '-d', '--seed', '0', '--level', 'info']
    coords = lambda out: [float(v) for v in re.findall(r'coords=(\S+?),?\s', out)]
    key_only = run(['train.py'] + _with_key(tmp_path, 'ciou') + tail + ['-n', 'key'])
    assert 'box_loss: ciou' in key_only, key_only[-2000:]
    flag_mse = run(['train.py'] + _with_key(tmp_path, 'ciou') + tail + ['-n', 'mse', '--box_loss', 'mse'])
    assert 'box_loss:' not in flag_mse and 'total_loss=' in flag_mse, flag_mse[-2000:]
    plain = run(['train.py'] + config(tmp_path, multiscale=None) + tail + ['-n', 'plain'])
    flag_giou = run(['train.py'] + _with_key(tmp_path, 'ciou') + tail + ['-n', 'giou', '--box_loss', 'giou'])
    assert 'box_loss: giou' in flag_giou and 'box_loss: ciou' not in flag_giou, flag_giou[-2000:]
    # the loss that ran, not only the line that was logged: same seed and data, so --box_loss mse over the key reports the plain run's `coords`
    # objective (up to the forward's summation order), and 1 - CIoU or 1 - GIoU is another quantity altogether
    c_key, c_mse, c_plain, c_giou = coords(key_only), coords(flag_mse), coords(plain), coords(flag_giou)
    assert c_key and c_mse and c_plain and c_giou, (key_only[-1500:], flag_mse[-1500:])
    print('coords: key ciou %r, key ciou + flag mse %r, plain %r, key ciou + flag giou %r' % (c_key, c_mse, c_plain, c_giou))
    assert len(c_mse) == len(c_plain) == len(c_key) == len(c_giou)
    assert np.allclose(c_mse, c_plain, rtol=1e-2, atol=2e-6)             # (six printed decimals)
    assert not np.allclose(c_key, c_plain, rtol=0.05, atol=2e-6) and not np.allclose(c_giou, c_plain, rtol=0.05, atol=2e-6)
    assert not np.allclose(c_giou, c_key, rtol=1e-3, atol=2e-6)


def test_unknown_value_and_yolo_v1_are_refused(tmp_path):
    tail = ['--data', 'synthetic', '-b', '2', '-s', '2', '--seed', '0', '-n', 'refused', '--level', 'info']
    out = run(['train.py'] + config(tmp_path, multiscale=None) + tail + ['--box_loss', 'l1'], ok=False)
    assert 'invalid choice' in out and "'l1'" in out and 'total_loss' not in out, out[-2000:]
    out = run(['train.py'] + config(tmp_path, multiscale=None, model='config/yolo/tiny-20.ini') + tail + ['--box_loss', 'giou'], ok=False)
    assert 'ValueError' in out and '[mi355x] box_loss = giou' in out and 'YOLO (v1)' in out, out[-2000:]
    assert 'total_loss' not in out and not os.path.exists(str(tmp_path / 'yolo'))       # no step, no logdir: nothing ran
