"""`train.py --ignore_thresh T --rescore --class_loss MODE --label_smoothing E --focal_gamma G` as a user runs it: a short run logs the options in
effect and finite losses; a value out of range and the YOLO (v1) family are refused before anything is built."""
import os
import re

import numpy as np
import pytest

from test_multiscale_cli_gpu import config, run

pytestmark = pytest.mark.gpu
TAIL = ['--data', 'synthetic', '-b', '2', '-s', '2', '--seed', '0', '--level', 'info']


def test_train_with_the_options(tmp_path):
    cfg = config(tmp_path, multiscale=None)
    out = run(['train.py'] + cfg + TAIL + ['-d', '-n', 'run0', '--ignore_thresh', '0.6', '--rescore', '--class_loss', 'ce', '--label_smoothing', '0.1'])
    assert 'loss options: class_loss=ce, ignore_thresh=0.6, rescore=True, label_smoothing=0.1' in out, out[-2000:]
    losses = [float(v) for v in re.findall(r'total_loss=(\S+)', out)]
    assert losses and np.all(np.isfinite(losses)), out[-2000:]
    assert 'model.ckpt-2' in out


def test_bad_values_and_yolo_v1_are_refused(tmp_path):
    tail = TAIL + ['-n', 'refused']
    out = run(['train.py'] + config(tmp_path, multiscale=None) + tail + ['--class_loss', 'bce'], ok=False)
    assert 'invalid choice' in out and 'total_loss' not in out, out[-2000:]
    out = run(['train.py'] + config(tmp_path, multiscale=None) + tail + ['--ignore_thresh', '1.5'], ok=False)
    assert 'ValueError' in out and 'ignore_thresh' in out and 'total_loss' not in out, out[-2000:]
    out = run(['train.py'] + config(tmp_path, multiscale=None, model='config/yolo/tiny-20.ini') + tail + ['--class_loss', 'focal'], ok=False)
    assert 'ValueError' in out and '[mi355x] class_loss = focal' in out and 'YOLO (v1)' in out, out[-2000:]
    assert 'total_loss' not in out and not os.path.exists(str(tmp_path / 'yolo'))       # no step, no logdir: nothing ran
