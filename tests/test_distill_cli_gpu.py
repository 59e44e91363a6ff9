"""train.py --teacher: a tiny-20 student distilled from a tiny-20 teacher that a three-step run wrote into a temporary directory; the four distill
scalars reach the log and the event file; a teacher without a checkpoint is an error that says so."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 64
MODEL = 'config/yolo2/tiny-20.ini'


def run(cmd, timeout=300):
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=timeout)
    return r.returncode, r.stdout + r.stderr


def overlay(tmp, name):
    path = tmp / (name + '.ini')
    path.write_text('[config]\nbasedir = %s\n[yolo2]\nwidth = %d\nheight = %d\n' % (tmp / name, SIZE, SIZE))
    return ['config.ini', MODEL, str(path)]


@pytest.mark.timeout_s(900)
def test_train_with_a_teacher(tmp_path):
    teacher, student = overlay(tmp_path, 'teacher'), overlay(tmp_path, 'student')
    common = ['--data', 'synthetic', '-b', '2', '-s', '3', '-d', '-n', 'run0', '--level', 'info']
    distilled = ['train.py', '-c'] + student + common + ['--seed', '1', '--teacher'] + teacher + ['--distill_class_term', 'kl', '--distill_temperature', '2']
    # no teacher checkpoint yet: an error that says so, before the student trains
    rc, out = run(distilled)
    assert rc != 0 and 'distillation needs a trained teacher: no teacher checkpoint in' in out and 'step 3:' not in out, out[-3000:]
    rc, out = run(['train.py', '-c'] + teacher + common + ['--seed', '2'])
    assert rc == 0 and glob.glob(str(tmp_path / 'teacher' / 'yolo2' / 'tiny' / '20' / 'model.ckpt-3.npz')), out[-3000:]
    rc, out = run(distilled)
    assert rc == 0, out[-3000:]
    assert 'distillation: teacher tiny (bf16) from' in out and 'model.ckpt-3.npz (global_step=3)' in out and 'class_term=kl, temperature=2.0' in out, out[-3000:]
    m = re.search(r'step 3: distill=(\S+) distill_objectness=(\S+) distill_coords=(\S+) distill_prob=(\S+)', out)
    assert m, out[-3000:]
    logged = [float(v) for v in m.groups()]
    assert np.isfinite(logged).all() and logged[0] > 0
    assert logged[0] == pytest.approx(sum(logged[1:]), rel=1e-4)               # every weight is 1
    from yolo_tf_amd.utils import events
    (path,) = glob.glob(str(tmp_path / 'student' / 'yolo2' / 'tiny' / '20' / 'run0' / 'events.out.tfevents.*'))
    scalars = {}
    for ev in events.read_events(path):
        scalars.update(dict(ev['scalars']))
    for tag, value in zip(('total_loss/distill', 'total_loss/distill/objectness', 'total_loss/distill/coords', 'total_loss/distill/prob'), logged):
        assert scalars[tag] == pytest.approx(value, rel=1e-4, abs=1e-6), tag
    # the teacher is not part of the student's checkpoint: the same variables as a run without one
    with np.load(str(tmp_path / 'student' / 'yolo2' / 'tiny' / '20' / 'model.ckpt-3.npz')) as z, \
            np.load(str(tmp_path / 'teacher' / 'yolo2' / 'tiny' / '20' / 'model.ckpt-3.npz')) as zt:
        assert sorted(z.files) == sorted(zt.files)
    # a named checkpoint that does not exist says so too
    rc, out = run(distilled + ['--teacher_ckpt', str(tmp_path / 'nowhere.npz')])
    assert rc != 0 and 'nowhere.npz does not exist' in out, out[-3000:]
