"""The evaluator without a GPU: the NumPy checker on hand cases whose answers are written out here, the host-only queries and
argument checks of the C ABI, the CLI's import safety and the .npz loader."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import eval_ref
from eval_ref import FP, IGNORED, TP
from yolo_tf_amd import evaluate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_checker_and_package_agree_on_the_record_format():
    assert (evaluate.FP, evaluate.TP, evaluate.IGNORED) == (FP, TP, IGNORED) == (0, 1, 2)
    assert evaluate.RECORD_DTYPE.itemsize == 16 and evaluate.RECORD_DTYPE.names == ('score', 'image', 'box', 'class_flag')


def test_worked_example_of_the_rules():
    # one class, two images, IoU threshold 0.5.  Image 0: A = [0,0,10,10], B = [20,0,30,10] (difficult); image 1: C = [0,0,10,10]
    gt_class = np.zeros(3, np.int32)
    gt_box = np.array([[0, 0, 10, 10], [20, 0, 30, 10], [0, 0, 10, 10]], np.float32)
    gt_difficult = np.array([0, 1, 0], np.uint8)
    gt_first = np.array([0, 2, 3], np.int32)
    boxes = np.zeros((2, 3, 4), np.float32)
    conf = np.zeros((2, 3, 1), np.float32)
    boxes[0, 0], conf[0, 0] = [0, 0, 10, 8], 0.9          # IoU 0.8 with A: TP
    boxes[0, 1], conf[0, 1] = [0, 0, 10, 6], 0.8          # IoU 0.6 with A: duplicate, FP
    boxes[0, 2], conf[0, 2] = [20, 0, 30, 7], 0.7         # IoU 0.7 with B (difficult): ignored
    boxes[1, 0], conf[1, 0] = [0, 0, 10, 3], 0.6          # IoU 0.3 with C: FP
    boxes[1, 1], conf[1, 1] = [0, 0, 10, 9], 0.5          # IoU 0.9 with C: TP
    for mode in ('detect', 'all'):
        records, npos = eval_ref.collect(conf, boxes[..., :2], boxes[..., 2:], gt_class, gt_box, gt_difficult, gt_first, 0, 2, 0.1, 0.5, mode)
        assert [r[2] for r in records] == [TP, FP, IGNORED, FP, TP]
        assert [(r[3], r[4]) for r in records] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)]
        assert list(npos) == [2]
        out = eval_ref.evaluate(records, npos, 1)
        assert out['order'][0].tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]]          # TP, FP, FP, TP
        assert out['cum_tp'][0].tolist() == [1, 1, 1, 2] and out['cum_fp'][0].tolist() == [0, 1, 2, 2]
        assert out['ap12'][0] == pytest.approx(0.75, abs=1e-15) and out['ap07'][0] == pytest.approx(8.5 / 11, abs=1e-15)
        assert (out['tp'], out['fp'], out['ignored'], out['detections']) == ([2], [2], [1], 5)


def test_iou_exactly_at_the_threshold_is_not_a_match():
    assert eval_ref.iou([0, 0, 2, 1], [0, 0, 1, 1]) == np.float32(0.5)
    conf = np.full((1, 1, 1), 0.9, np.float32)
    box = np.array([[[0, 0, 2, 1]]], np.float32)
    args = (np.zeros(1, np.int32), np.array([[0, 0, 1, 1]], np.float32), np.zeros(1, np.uint8), np.array([0, 1], np.int32), 0, 1, 0.1)
    records, npos = eval_ref.collect(conf, box[..., :2], box[..., 2:], *args, 0.5, 'detect')
    assert [r[2] for r in records] == [FP] and list(npos) == [1]
    out = eval_ref.evaluate(records, npos, 1)
    assert out['ap07'] == [0.0] and out['ap12'] == [0.0]
    records, _ = eval_ref.collect(conf, box[..., :2], box[..., 2:], *args, 0.4999, 'detect')        # just below: a match
    assert [r[2] for r in records] == [TP]


def test_score_ties_break_by_image_then_box():
    # (score, class, flag, image, box): four records of one score, emitted out of order
    records = [(np.float32(0.5), 0, FP, 1, 0), (np.float32(0.5), 0, TP, 0, 7), (np.float32(0.5), 0, FP, 0, 3), (np.float32(0.5), 0, TP, 1, 2),
               (np.float32(0.75), 0, FP, 9, 9)]
    out = eval_ref.evaluate(records, np.array([2]), 1)
    assert out['order'][0].tolist() == [[9, 9], [0, 3], [0, 7], [1, 0], [1, 2]]          # FP, FP, TP, FP, TP
    assert out['cum_tp'][0].tolist() == [0, 0, 1, 1, 2] and out['cum_fp'][0].tolist() == [1, 2, 2, 3, 3]
    # precision at the two TPs: 1/3 and 2/5; the envelope lifts the first to 2/5: ap12 = 0.5 * 0.4 + 0.5 * 0.4
    assert out['ap12'][0] == pytest.approx(0.4, abs=1e-15)
    assert out['ap07'][0] == pytest.approx(0.4, abs=1e-15)                              # every threshold sees the point (recall 1, precision 0.4)


def test_class_without_ground_truth_is_nan_and_left_out_of_the_mean():
    records = [(np.float32(0.9), 0, TP, 0, 0), (np.float32(0.8), 1, FP, 0, 1)]
    out = eval_ref.evaluate(records, np.array([1, 0, 3]), 3)
    assert out['ap07'][0] == 1.0 and out['ap12'][0] == 1.0
    assert math.isnan(out['ap07'][1]) and math.isnan(out['ap12'][1])                      # npos == 0, although it has a detection
    assert out['ap07'][2] == 0.0 and out['ap12'][2] == 0.0                                # npos > 0, no detection
    assert out['mAP07'] == 0.5 and out['mAP12'] == 0.5
    assert math.isnan(eval_ref.evaluate([], np.zeros(2, np.int64), 2)['mAP07'])


def test_record_and_workspace_queries():
    from yolo_tf_amd import _lib
    q = _lib.query
    assert q('yolo2_eval_record_bytes', 1000) == 16 * 1000
    assert q('yolo2_eval_collect_workspace_bytes', 256) == 4 * 256
    assert q('yolo2_eval_result_bytes', 20) == 8 * (6 * 20 + 3)
    # two record buffers + one 256-digit row per 16384-record tile, each rounded up to 256 bytes
    assert q('yolo2_eval_workspace_bytes', 1000, 20) == 2 * 16128 + 1024
    assert q('yolo2_eval_workspace_bytes', 4952 * 845, 20) == 2 * (4952 * 845 * 16 + 128) + 256 * 256 * 4        # (66951040 -> 66951168)
    assert q('yolo2_eval_workspace_bytes', 0, 20) == 0 and q('yolo2_eval_record_bytes', 0) == 0


def test_bad_arguments_raise_without_a_gpu():
    from yolo_tf_amd import _lib
    p = 4096           # stands for a device pointer: the checks come before anything is launched
    good = dict(conf=p, xy_min=p, xy_max=p, gt_class=p, gt_box=p, gt_difficult=p, gt_first=p, G=1, B=2, N=10, C=3, n_valid=2, image_base=0,
                mode=0, thr=0.1, iou=0.5, records=p, cap=100, state=p, npos=p, ws=p)

    def collect(**kw):
        a = dict(good, **kw)
        _lib.call('yolo2_eval_collect', *[a[k] for k in good], None)
    for bad in (dict(conf=None), dict(gt_first=None), dict(records=None), dict(state=None), dict(npos=None), dict(ws=None), dict(C=0), dict(C=-1),
                dict(cap=0), dict(mode=2), dict(mode=-1), dict(n_valid=3), dict(B=0), dict(N=0), dict(image_base=-1), dict(thr=float('nan'))):
        with pytest.raises(_lib.HipKernelError, match='argument check failed'):
            collect(**bad)
    ws_bytes = _lib.query('yolo2_eval_workspace_bytes', 100, 3)
    fgood = dict(records=p, cap=100, state=p, npos=p, C=3, n_images=4, N=10, ws=p, ws_bytes=ws_bytes, results=p)
    for bad in (dict(records=None), dict(state=None), dict(npos=None), dict(ws=None), dict(results=None), dict(C=0), dict(cap=0), dict(n_images=0),
                dict(N=0), dict(ws_bytes=ws_bytes - 1)):
        a = dict(fgood, **bad)
        with pytest.raises(_lib.HipKernelError, match='argument check failed'):
            _lib.call('yolo2_eval_finalize', *[a[k] for k in fgood], None, None, None, None)


def test_evaluator_rejects_an_unknown_mode():
    from yolo_tf_amd import evaluate
    with pytest.raises(ValueError, match='mode'):
        evaluate.Evaluator(20, 100, mode='coco', device='cpu')


def test_cli_help_and_import_have_no_side_effects(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'eval.py'), '--help'], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and '--threshold_iou' in r.stdout and '--mode' in r.stdout and '--json' in r.stdout, r.stderr[-2000:]
    code = 'import sys, os; before = set(os.listdir(".")); import eval; assert callable(eval.main) and callable(eval.make_args); ' \
           'assert "torch" not in sys.modules; assert set(os.listdir(".")) == before; print("ok")'
    r = subprocess.run([sys.executable, '-c', code], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stderr[-2000:]
    assert os.listdir(str(tmp_path)) == []


def test_npz_without_difficult_flags_loads_zeros(tmp_path):
    from yolo_tf_amd import evaluate
    images = np.empty(2, object)
    images[0], images[1] = np.zeros((4, 6, 3), np.uint8), np.zeros((5, 3, 3), np.uint8)
    z = dict(images=images, objects_class=np.array([1, 2, 0], np.int32), objects_coord=np.arange(12, dtype=np.float32).reshape(3, 4),
             objects_first=np.array([0, 2, 3], np.int32))
    np.savez(str(tmp_path / 'a.npz'), **z)
    imgs, objects, difficult = evaluate.load_npz(str(tmp_path / 'a.npz'))
    assert len(imgs) == 2 and [len(c) for c, _ in objects] == [2, 1]
    assert [d.tolist() for d in difficult] == [[0, 0], [0]] and all(d.dtype == np.uint8 for d in difficult)
    np.savez(str(tmp_path / 'b.npz'), objects_difficult=np.array([0, 1, 1], np.uint8), **z)
    assert [d.tolist() for d in evaluate.load_npz(str(tmp_path / 'b.npz'))[2]] == [[0, 1], [1]]
    # ground truth in cell units: pixels * cells / image size, float32
    gt = evaluate.gt_in_cells(objects, [(6, 4), (3, 5)], 13, 13, difficult)
    np.testing.assert_array_equal(gt[0][1], (np.arange(8, dtype=np.float32).reshape(2, 4) * np.array([13 / 6, 13 / 4] * 2, np.float32)).astype(np.float32))
