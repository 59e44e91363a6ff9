"""`[mi355x] multiscale`, `--multiscale` and `eval.py --sizes` as a user runs them: train with the key and resume the schedule, evaluate the one
checkpoint at two sizes against single-size runs, and be refused where multi-scale training cannot work."""
import json
import math
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


def write_raw_objects(path):
    """The raw-object layout of train.py --data file.npz: decoded images and their boxes in pixels."""
    rng = np.random.RandomState(6)
    images = rng.randint(0, 256, (6, 90, 120, 3)).astype(np.uint8)
    cls, coord, first = [], [], [0]
    for _ in images:
        k = rng.randint(1, 4)
        x0, y0 = rng.uniform(0, 60, k), rng.uniform(0, 45, k)
        cls.append(rng.randint(0, 20, k))
        coord.append(np.stack([x0, y0, x0 + rng.uniform(8, 48, k), y0 + rng.uniform(8, 36, k)], 1))
        first.append(first[-1] + k)
    np.savez(str(path), images=images, objects_class=np.concatenate(cls).astype(np.int32), objects_coord=np.concatenate(coord).astype(np.float32),
             objects_first=np.asarray(first, np.int32))
    return str(path)


def config(tmp, name='local.ini', size=96, multiscale='64-128', model=MODEL):
    overlay = tmp / name
    section = 'yolo' if '/yolo/' in model else 'yolo2'
    text = '[config]\nbasedir = %s\n[%s]\nwidth = %d\nheight = %d\n' % (tmp, section, size, size)
    if multiscale:
        text += '[mi355x]\nmultiscale = %s\nmultiscale_every = 2\n' % multiscale
    overlay.write_text(text)
    return ['-c', 'config.ini', model, str(overlay)]


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """Six steps of `train.py` with the key set: (directory, data file, config arguments, the run's output)."""
    tmp = tmp_path_factory.mktemp('multiscale_cli')
    data = write_raw_objects(tmp / 'raw.npz')
    cfg = config(tmp)
    out = run(['train.py'] + cfg + ['--data', data, '-b', '2', '-s', '6', '-d', '--seed', '0', '-n', 'run0', '--level', 'info'])
    return tmp, data, cfg, out


def size_lines(out):
    return [line.split('step ', 1)[1] for line in out.splitlines() if ': input size ' in line]


def test_train_logs_the_list_and_the_size_changes_then_resumes_the_schedule(trained):
    tmp, data, cfg, out = trained
    assert 'multiscale: sizes 64 96 128, a new draw every 2 steps' in out, out[-2000:]
    assert 'is added' not in out                                          # 96 is a member of 64-128
    assert size_lines(out) == ['0: input size 64x64', '2: input size 96x96', '4: input size 64x64'], out[-2000:]
    assert 'model.ckpt-6' in out and 'total_loss=' in out and 'total_loss=nan' not in out
    out = run(['train.py'] + cfg + ['--data', data, '-b', '2', '-s', '8', '--seed', '0', '-n', 'run1', '--level', 'info'])
    assert 'global_step=6' in out and size_lines(out) == ['6: input size 128x128'], out[-2000:]
    assert 'model.ckpt-8' in out


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return type(a) is type(b) and a == b


def test_eval_at_two_sizes_equals_two_single_size_runs(trained):
    tmp, _, cfg, _ = trained
    # Inference is not bitwise repeatable (tests/test_multiscale_gpu.py, SPREAD), so two runs of eval.py could in principle differ.  Measured: six
    # single-size runs of exactly these commands at each of the two sizes wrote one and the same result (profiles/multiscale.md) -- a spread of zero,
    # and twice zero is what is allowed here: equality.
    common = ['--data', 'synthetic', '--images', '4', '-b', '4']
    path = tmp / 'sizes.json'
    out = run(['eval.py'] + cfg + common + ['--sizes', '64 128', '--json', str(path)])
    assert 'size 64x64' in out and 'size 128x128' in out and 'ms/batch' in out, out[-2000:]
    assert out.index('size 64x64') < out.index('size 128x128') < out.index('ms/batch')
    r = json.loads(path.read_text())
    assert sorted(r['by_size']) == ['128x128', '64x64'] and r['sizes'] == ['64x64', '128x128']
    assert all(r['ms_per_batch'][k] > 0 for k in r['by_size'])
    for k in ('names', 'images', 'checkpoint', 'global_step', 'config', 'ema'):
        assert k in r, k
    for size in (64, 128):
        single_path = tmp / ('single_%d.json' % size)
        single_cfg = config(tmp, 'single%d.ini' % size, size=size, multiscale=None)
        out = run(['eval.py'] + single_cfg + common + ['--json', str(single_path)])
        assert 'size ' not in out and 'ms/batch' not in out                # without the flag the output is what it was
        single = json.loads(single_path.read_text())
        assert 'by_size' not in single and single['checkpoint'] == r['checkpoint'] and single['global_step'] == r['global_step']
        entry = r['by_size']['%dx%d' % (size, size)]
        assert 'ap07' in entry and 'mAP12' in entry and 'npos' in entry and 'detections' in entry
        assert same(entry, {k: single[k] for k in entry}), (size, entry, {k: single.get(k) for k in entry})
        assert sorted(set(single) - set(entry)) == sorted(set(r) - {'by_size', 'sizes', 'ms_per_batch'})
    assert r['by_size']['64x64']['detections'] > 0 and r['by_size']['64x64'] != r['by_size']['128x128']


def test_refusals_exit_non_zero_before_any_step(trained, tmp_path):
    tmp, data, cfg, _ = trained
    tail = ['-b', '2', '-s', '2', '--seed', '0', '-n', 'refused', '--level', 'info']
    # the YOLO (v1) family: its fully connected head fixes the size
    out = run(['train.py'] + config(tmp_path, model='config/yolo/tiny-20.ini', size=448, multiscale='448') + ['--data', 'synthetic'] + tail, ok=False)
    assert 'ValueError' in out and '[mi355x] multiscale' in out and 'fully connected' in out, out[-2000:]
    # ready-made label tensors: laid out for one grid
    from yolo_tf_amd.utils import data as udata
    labels = udata.synthetic_batch(4, 20, 3, 3, seed=0)
    ready = tmp_path / 'labels.npz'
    np.savez(str(ready), images=np.zeros((4, 96, 96, 3), np.uint8), **dict(zip(udata.LABEL_KEYS, labels)))
    out = run(['train.py'] + config(tmp_path) + ['--data', str(ready)] + tail, ok=False)
    assert 'ValueError' in out and '[mi355x] multiscale' in out and 'ready-made label tensors' in out, out[-2000:]
    # a size that is no multiple of the stride, from the flag
    out = run(['train.py'] + config(tmp_path, multiscale=None) + ['--data', data, '--multiscale', '100'] + tail, ok=False)
    assert 'ValueError' in out and '[mi355x] multiscale' in out and "'100'" in out and '32' in out, out[-2000:]
    assert not os.path.exists(str(tmp_path / 'yolo2')) and not os.path.exists(str(tmp_path / 'yolo'))      # no logdir, no checkpoint: nothing ran
