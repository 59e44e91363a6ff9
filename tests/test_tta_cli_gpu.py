"""eval.py --tta and detect.py --tta end to end on the MI355X: two steps of train.py on the tiny network at 64 x 64, then the two tools on its
checkpoint.  (The tools are what is tested here, so this file starts processes; the kernels and the session are tested in
tests/test_tta_gpu.py and tests/test_tta_session_gpu.py.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = 'config/yolo2/tiny-20.ini'
SIZE = 64
pytestmark = pytest.mark.gpu


def run(cmd, timeout=600, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert (r.returncode == 0) == ok, 'exit %d: %s\n--- stdout\n%s\n--- stderr\n%s' % (r.returncode, ' '.join(cmd), r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout + r.stderr


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """Two steps of train.py on the tiny network at 64 x 64: (directory, config arguments)."""
    tmp = tmp_path_factory.mktemp('tta_cli')
    overlay = tmp / 'local.ini'
    overlay.write_text('[config]\nbasedir = %s\n[yolo2]\nwidth = %d\nheight = %d\n' % (tmp, SIZE, SIZE))
    cfg = ['-c', 'config.ini', MODEL, str(overlay)]
    run(['train.py'] + cfg + ['--data', 'synthetic', '-b', '2', '-s', '2', '-d', '--seed', '1', '-n', 'run0', '--level', 'info'])
    return tmp, cfg


def test_eval_cli_fuses_views_and_records_them(trained):
    tmp, cfg = trained
    common = ['--data', 'synthetic', '--images', '4', '-b', '4', '--mode', 'all']
    path = tmp / 'tta.json'
    out = run(['eval.py'] + cfg + common + ['--tta', 'flip 96', '--json', str(path)])
    assert 'mAP07' in out and 'global_step=2' in out and 'views 64 96 64+flip 96+flip' in out, out[-2000:]
    got = json.loads(path.read_text())
    assert got['config']['tta'] == '64 96 64+flip 96+flip' and got['config']['tta_iou'] == 0.55 and got['detections'] > 0
    # [mi355x] tta / tta_iou are read; a flag wins
    key = tmp / 'tta.ini'
    key.write_text('[mi355x]\ntta = flip\ntta_iou = 0.6\n')
    run(['eval.py'] + cfg + [str(key)] + common + ['--tta_iou', '0.5', '--json', str(path)])
    got = json.loads(path.read_text())['config']
    assert (got['tta'], got['tta_iou']) == ('64 64+flip', 0.5)


def test_eval_cli_refuses_tta_with_sizes_and_a_bad_token(trained):
    tmp, cfg = trained
    common = ['--data', 'synthetic', '--images', '4', '-b', '4']
    out = run(['eval.py'] + cfg + common + ['--tta', 'flip', '--sizes', '64 96'], ok=False)
    assert 'one table per input size' in out and 'one result' in out
    out = run(['eval.py'] + cfg + common + ['--tta', 'flip mirror'], ok=False)
    assert "'mirror'" in out


def test_detect_cli_prints_fused_detections(trained):
    from PIL import Image
    tmp, cfg = trained
    # a uniform grey image: two steps in, a textured one overflows this network's box decode and detect.py raises, as it should (tests/test_ema_cli_gpu.py)
    img = tmp / 'img.png'
    Image.fromarray(np.full((90, 120, 3), 128, np.uint8)).save(str(img))
    out = run(['detect.py', str(img)] + cfg + ['-t', '0.000001', '--level', 'info', '--tta', 'flip'])
    assert 'objects detected' in out and 'views 64 64+flip' in out and 'global_step=2' in out, out[-2000:]
    lines = [l for l in out.splitlines() if l.startswith('  ') and '%' in l]
    scores = [float(l.split()[1].rstrip('%')) for l in lines]
    assert len(lines) > 0 and scores == sorted(scores, reverse=True)      # best fused score first
