"""Soft-NMS through the public surface: DetectSession.detect / nms, evaluate.evaluate and the two CLIs, at 64 x 64 on the tiny network
with seeded random weights.  The expected scores are the specification's (tests/soft_nms_ref.py) applied to a clone of the buffers the NMS
is given, bit for bit, order included.

Random weights can overflow the box decoder's exp(); boxes that are not finite are outside the specification (and the kernel's fminf /
fmaxf and NumPy's minimum / maximum treat NaN differently), so a hook in front of the session's NMS replaces them, as
tests/test_eval_coco_gpu.py's FiniteBoxes does behind it, and clones what the NMS then sees."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import soft_nms_ref as S
from soft_nms_cases import bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = 'config/yolo2/tiny-20.ini'
SIZE = 64


def make_builder(size, basedir):
    from yolo_tf_amd import utils
    from yolo_tf_amd.model import yolo2
    cfg = utils.make_config([os.path.join(ROOT, 'config.ini'), os.path.join(ROOT, MODEL)], basedir)
    cfg.set('cache', 'names', os.path.join(ROOT, cfg.get('cache', 'names')))
    cfg.set('yolo2', 'anchors', os.path.join(ROOT, cfg.get('yolo2', 'anchors')))
    cfg.set('yolo2', 'width', str(size))
    cfg.set('yolo2', 'height', str(size))
    utils.ensure_names(cfg)
    b = yolo2.Builder(None, cfg)
    b(None)
    return b


def hook_nms(sess):
    """Puts a recorder in front of sess.nms (detect() calls it through the instance): non-finite boxes and scores are replaced in place, then
    the buffers are cloned to the host, then the session's own nms runs.  Returns the list the clones are appended to."""
    seen = []
    original = sess.nms

    def nms(*args, **kw):
        for t in (sess.xy_min, sess.xy_max):
            torch.nan_to_num_(t, nan=0.0, posinf=1e4, neginf=-1e4)
            t.clamp_(-1e4, 1e4)
        torch.nan_to_num_(sess.conf, nan=0.0, posinf=1.0, neginf=0.0)
        assert bool((sess.xy_min <= sess.xy_max).all().item())
        seen.append((sess.conf.cpu().numpy().copy(), sess.xy_min.cpu().numpy().copy(), sess.xy_max.cpu().numpy().copy()))
        return original(*args, **kw)
    sess.nms = nms
    return seen


@pytest.fixture(scope='module')
def session():
    from yolo_tf_amd.session import DetectSession
    with tempfile.TemporaryDirectory() as basedir:
        builder = make_builder(SIZE, basedir)
        sess = DetectSession(builder, 4, dtype='bf16', seed=4)
        yield builder, sess


def images(seed, batch=4):
    return torch.from_numpy(np.random.RandomState(seed).uniform(0, 255, (batch, SIZE, SIZE, 3)).astype(np.float32)).cuda()


def test_detect_gaussian_equals_the_specification(session):
    _, sess = session
    seen = hook_nms(sess)
    try:
        # threshold 0: random weights give peaked class scores (most are far below any usual threshold, and the few above it do not
        # overlap); with every positive score a candidate, the anchors of a cell decay each other, down into the subnormal range
        thr, thr_iou, sigma = 0.0, 0.45, 0.5
        conf, xy_min, xy_max, order = sess.detect(images(1), thr, thr_iou, 0, nms='gaussian', sigma=sigma)
        torch.cuda.synchronize()
        (conf0, mn0, mx0), = seen
        want, want_order = S.soft_nms(conf0, mn0, mx0, thr, thr_iou, 'gaussian', sigma)
        assert ((conf0 > np.float32(thr)).sum(axis=1) >= 2).any()                                   # a class with two candidates: a decay is possible
        assert not np.array_equal(bits(want), bits(conf0))                                          # ... and it did something
        assert np.array_equal(bits(conf.cpu().numpy()), bits(want))
        assert np.array_equal(order.cpu().numpy(), want_order)
        assert np.array_equal(bits(xy_min.cpu().numpy()), bits(mn0)) and np.array_equal(bits(xy_max.cpu().numpy()), bits(mx0))
        # the session's nms alone, linear, on the same buffers put back
        sess.conf.copy_(torch.from_numpy(conf0).cuda())
        order = sess.nms(thr, thr_iou, method='linear')
        want, want_order = S.soft_nms(conf0, mn0, mx0, thr, thr_iou, 'linear')
        assert np.array_equal(bits(sess.conf.cpu().numpy()), bits(want)) and np.array_equal(order.cpu().numpy(), want_order)
        with pytest.raises(ValueError):
            sess.nms(thr, thr_iou, method='softer')
    finally:
        del sess.nms


def test_detect_hard_is_detect_without_the_keyword(session):
    """nms='hard' goes to yolo2_nms exactly as before.  Inference is not bitwise repeatable from run to run, so run() is replaced by one that
    puts the same decoded buffers back: detect() as bench.py calls it (positionally) and detect(nms='hard') then give the same bits and order."""
    _, sess = session
    sess.run(images(2), 0, check_numerics=False)
    for t in (sess.xy_min, sess.xy_max):
        torch.nan_to_num_(t, nan=0.0, posinf=1e4, neginf=-1e4)
        t.clamp_(-1e4, 1e4)
    torch.nan_to_num_(sess.conf, nan=0.0, posinf=1.0, neginf=0.0)
    conf0, mn0, mx0 = sess.conf.clone(), sess.xy_min.clone(), sess.xy_max.clone()

    def run(*args, **kw):
        sess.conf.copy_(conf0)
        sess.xy_min.copy_(mn0)
        sess.xy_max.copy_(mx0)
        return sess.conf, sess.xy_min, sess.xy_max
    sess.run = run
    try:
        results = []
        for kw in ({}, {'nms': 'hard'}, {'nms': 'hard', 'sigma': 0.25}):
            out = sess.detect(images(2), 0.001, 0.45, 0, **kw)
            torch.cuda.synchronize()
            results.append([bits(t.cpu().numpy()) if t.dtype == torch.float32 else t.cpu().numpy().copy() for t in out])
        soft = [t.cpu().numpy().copy() for t in sess.detect(images(2), 0.001, 0.45, 0, nms='linear')]
    finally:
        del sess.run
    assert not np.array_equal(results[0][0], bits(conf0.cpu().numpy()))                 # the NMS did something
    for got in results[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(got, results[0]))
    want, want_order = S.soft_nms(conf0.cpu().numpy(), mn0.cpu().numpy(), mx0.cpu().numpy(), 0.001, 0.45, 'linear')
    assert np.array_equal(bits(soft[0]), bits(want)) and np.array_equal(soft[3], want_order)


def test_evaluate_linear_equals_an_evaluator_fed_the_specification(session):
    from yolo_tf_amd import evaluate
    builder, sess = session
    m = sess.model
    imgs, objects, difficult = evaluate.synthetic_dataset(8, 20, seed=9)
    data = evaluate.EvalData(imgs, objects, 4, builder.width, builder.height, m.cell_width, m.cell_height, difficult=difficult)
    # every positive score a candidate and every overlap decays (IoU >= 0): see above; at usual thresholds the few candidates random weights
    # leave do not overlap, and a suppression step that changes nothing could not tell linear from hard
    thr, thr_iou = 0.0, 0.0
    ev = evaluate.Evaluator(20, 8 * sess.N * 20, mode='all', threshold=thr, iou_threshold=0.5)
    seen = hook_nms(sess)
    batches, decayed = [], []
    try:
        def on_batch(s, gt, base, n_valid):
            conf0, mn0, mx0 = seen[-1]
            want, _ = S.soft_nms(conf0, mn0, mx0, thr, thr_iou, 'linear')
            assert np.array_equal(bits(s.conf.cpu().numpy()), bits(want))
            decayed.append(not np.array_equal(bits(want), bits(conf0)))
            ev.add(torch.from_numpy(want).cuda(), torch.from_numpy(mn0).cuda(), torch.from_numpy(mx0).cuda(), *gt, image_base=base, n_valid=n_valid)
            batches.append(base)
        res = evaluate.evaluate(builder, sess, data, mode='all', threshold=thr, threshold_iou=thr_iou, iou=0.5, on_batch=on_batch, nms='linear')
    finally:
        del sess.nms
    assert len(seen) == len(batches) == 2 and any(decayed)                  # the linear decay changed scores
    ref = ev.result()
    assert res['detections'] == ref['detections'] > 0
    for k in ('ap07', 'ap12', 'npos', 'tp', 'fp'):
        assert np.array_equal(np.asarray(res[k]), np.asarray(ref[k]), equal_nan=True), k


# ---------------------------------------------------------------------------------------------------------------------
# the CLIs
# ---------------------------------------------------------------------------------------------------------------------

def run(cmd, timeout=600, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert (r.returncode == 0) == ok, 'exit %d: %s\n--- stdout\n%s\n--- stderr\n%s' % (r.returncode, ' '.join(cmd), r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout + r.stderr


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """Two steps of train.py on the tiny network at 64 x 64: (directory, config arguments)."""
    tmp = tmp_path_factory.mktemp('soft_nms_cli')
    overlay = tmp / 'local.ini'
    overlay.write_text('[config]\nbasedir = %s\n[yolo2]\nwidth = %d\nheight = %d\n' % (tmp, SIZE, SIZE))
    cfg = ['-c', 'config.ini', MODEL, str(overlay)]
    run(['train.py'] + cfg + ['--data', 'synthetic', '-b', '2', '-s', '2', '-d', '--seed', '1', '-n', 'run0', '--level', 'info'])
    return tmp, cfg


def test_eval_cli_records_the_method(trained):
    tmp, cfg = trained
    common = ['--data', 'synthetic', '--images', '4', '-b', '4']
    soft_path, hard_path, ini_path = tmp / 'soft.json', tmp / 'hard.json', tmp / 'ini.json'
    out = run(['eval.py'] + cfg + common + ['--nms', 'gaussian', '--sigma', '0.5', '--json', str(soft_path)])
    assert 'mAP07' in out and 'global_step=2' in out, out[-2000:]
    soft = json.loads(soft_path.read_text())
    assert soft['config']['nms'] == 'gaussian' and soft['config']['sigma'] == 0.5
    run(['eval.py'] + cfg + common + ['--json', str(hard_path)])
    hard = json.loads(hard_path.read_text())
    assert hard['config']['nms'] == 'hard' and hard['config']['sigma'] == 0.5
    assert sorted(hard) == sorted(soft) and sorted(hard['config']) == sorted(soft['config'])      # the same keys with and without the flag
    # [mi355x] nms / nms_sigma are read; the flag wins
    key = tmp / 'nms.ini'
    key.write_text('[mi355x]\nnms = linear\nnms_sigma = 0.25\n')
    run(['eval.py'] + cfg + [str(key)] + common + ['--json', str(ini_path)])
    got = json.loads(ini_path.read_text())['config']
    assert (got['nms'], got['sigma']) == ('linear', 0.25)
    run(['eval.py'] + cfg + [str(key)] + common + ['--nms', 'gaussian', '--json', str(ini_path)])
    got = json.loads(ini_path.read_text())['config']
    assert (got['nms'], got['sigma']) == ('gaussian', 0.25)


def test_detect_cli_runs_with_linear_and_refuses_a_bad_method(trained):
    from PIL import Image
    tmp, cfg = trained
    # a uniform grey image: two steps in, a textured one overflows this network's box decode and detect.py raises, as it should (tests/test_ema_cli_gpu.py)
    img = tmp / 'img.png'
    Image.fromarray(np.full((90, 120, 3), 128, np.uint8)).save(str(img))
    out = run(['detect.py', str(img)] + cfg + ['-t', '0.000001', '--level', 'info', '--nms', 'linear'])
    assert 'objects detected' in out and 'global_step=2' in out, out[-2000:]
    out = run(['detect.py', str(img)] + cfg + ['--nms', 'softer'], ok=False)
    assert 'invalid choice' in out
    out = run(['eval.py'] + cfg + ['--data', 'synthetic', '--images', '4', '-b', '4', '--nms', 'softer'], ok=False)
    assert 'invalid choice' in out
    out = run(['eval.py'] + cfg + ['--data', 'synthetic', '--images', '4', '-b', '4', '--nms', 'gaussian', '--sigma', '0.001'], ok=False)
    assert 'yolo2_soft_nms' in out and 'argument check failed' in out, out[-2000:]
