"""`train.py --mosaic P --mixup P` as a user runs it: a short run on raw objects logs the setting and a finite loss (the pipeline's check
of the label kernel's error flag runs with the last step's summary and would end the run), and data without raw objects is refused before
any step."""
import os
import re

import numpy as np
import pytest

from test_multiscale_cli_gpu import config, run, write_raw_objects

pytestmark = pytest.mark.gpu


def test_train_with_mosaic_and_mixup(tmp_path):
    data = write_raw_objects(tmp_path / 'raw.npz')
    cfg = config(tmp_path, multiscale=None)
    out = run(['train.py'] + cfg + ['--data', data, '-b', '2', '-s', '4', '-d', '--seed', '0', '-n', 'run0', '--level', 'info', '--mosaic', '1', '--mixup', '0.5'])
    assert 'mosaic: probability 1, scale 0.5-1.5, fill 114; mixup: probability 0.5, alpha 1.5' in out, out[-2000:]
    losses = [float(v) for v in re.findall(r'total_loss=(\S+)', out)]
    assert losses and np.all(np.isfinite(losses)), out[-2000:]
    assert 'model.ckpt-4' in out and 'IndexError' not in out and 'AssertionError' not in out


def test_refused_without_raw_objects(tmp_path):
    tail = ['-b', '2', '-s', '2', '--seed', '0', '-n', 'refused', '--level', 'info']
    out = run(['train.py'] + config(tmp_path, multiscale=None) + ['--data', 'synthetic', '--mosaic', '1'] + tail, ok=False)
    assert 'ValueError' in out and '[mi355x] mosaic = 1' in out and 'holds no raw objects' in out, out[-2000:]
    assert 'total_loss' not in out and not os.path.exists(str(tmp_path / 'yolo2'))       # no step, no logdir: nothing ran
    out = run(['train.py'] + config(tmp_path, multiscale=None) + ['--data', 'synthetic', '--mixup', '1.5'] + tail, ok=False)
    assert 'ValueError' in out and '[mi355x] mixup' in out, out[-2000:]
