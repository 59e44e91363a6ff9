"""Dimension clusters without a GPU: known answers of the NumPy specification (tests/anchors_ref.py), the host functions that turn a
dataset into boxes in cell units, the anchor TSV round trip, the command line's argument rules and the argument checks of the new C ABI
entries (which return before anything is launched)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anchors_ref as R  # noqa: E402

from yolo_tf_amd import anchors as A  # noqa: E402
from yolo_tf_amd import utils  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).tolist()


# ---------------------------------------------------------------- the specification's known answers
def quantised_mean(v):
    """(float)((double)sum of rint(v * 2^24) / count * 2^-24), in exact integer arithmetic up to the one division."""
    s = sum(int(np.rint(np.float64(x) * 2.0 ** 24)) for x in np.asarray(v, np.float32))
    return np.float32(np.float64(s) / np.float64(len(v)) * 2.0 ** -24)


def test_two_separated_groups_give_their_quantised_means():
    rng = np.random.RandomState(3)
    small = (np.array([1.0, 1.5]) + rng.uniform(-0.05, 0.05, (40, 2))).astype(np.float32)
    large = (np.array([8.0, 6.0]) + rng.uniform(-0.05, 0.05, (25, 2))).astype(np.float32)
    boxes = np.concatenate([small, large])[rng.permutation(65)]
    first_small = int(np.argmax(boxes[:, 0] < 4)), int(np.argmax(boxes[:, 0] > 4))
    cen, iterations, converged = R.fit(boxes, boxes[list(first_small)], 50)
    assert converged and iterations <= 3
    want = np.array([[quantised_mean(small[:, 0]), quantised_mean(small[:, 1])], [quantised_mean(large[:, 0]), quantised_mean(large[:, 1])]], np.float32)
    assert bits(cen) == bits(want)
    avg, counts, arg = R.score(boxes, cen)
    assert counts.tolist() == [40, 25] and (arg == (boxes[:, 0] > 4)).all()
    # average IoU against an independent f64 evaluation: every f32 operation is within 2^-24 relative, the fixed point adds 2^-31 per box
    b, c = boxes.astype(np.float64), cen.astype(np.float64)[arg]
    inter = np.minimum(b[:, 0], c[:, 0]) * np.minimum(b[:, 1], c[:, 1])
    exact = np.mean(inter / (b[:, 0] * b[:, 1] + c[:, 0] * c[:, 1] - inter))
    assert abs(avg - exact) < 1e-6
    # ... and to 1e-12 against the fixed-point sum redone with Python integers (round() is half to even) from the same f32 IoUs
    m = R.iou(boxes, cen)
    fixed = sum(round(float(v) * 2 ** 30) for v in m[np.arange(len(boxes)), arg])
    assert abs(avg - fixed / 2 ** 30 / len(boxes)) < 1e-12


def test_k1_gives_the_global_mean():
    rng = np.random.RandomState(4)
    boxes = np.exp(rng.normal(1.0, 0.6, (257, 2))).astype(np.float32)
    cen, iterations, converged = R.fit(boxes, boxes[:1], 10)
    assert converged and iterations == 2          # the first update moves to the mean, the second finds it unchanged
    assert bits(cen) == bits([[quantised_mean(boxes[:, 0]), quantised_mean(boxes[:, 1])]])


def test_duplicate_initial_centroids_leave_the_higher_index_empty_and_unchanged():
    rng = np.random.RandomState(5)
    boxes = np.exp(rng.normal(1.0, 0.6, (300, 2))).astype(np.float32)
    init = np.stack([boxes[7], boxes[100], boxes[7]])
    new, count, _, arg = R.step(boxes, init)
    assert count[2] == 0 and not (arg == 2).any()
    assert bits(new[2]) == bits(init[2]) and bits(new[0]) != bits(init[0])          # (after that step the two differ, and index 2 is an ordinary centroid)


# ---------------------------------------------------------------- boxes of a dataset
SAMPLES = [      # (path, (h, w, c), classes, coords xmin ymin xmax ymax in pixels)
    ('a.jpg', (100, 200, 3), [1, 2], [[10, 20, 110, 70], [0, 0, 200, 100]]),
    ('b.jpg', (416, 416, 3), [0], [[16, 32, 48, 96]]),
    ('c.jpg', (50, 40, 3), [], np.zeros((0, 4), np.float32)),
]
WANT_13 = np.array([[100 / 200 * 13, 50 / 100 * 13], [13, 13], [32 / 416 * 13, 64 / 416 * 13]], np.float32)          # by hand: extent / image * 13


def test_boxes_in_cells_from_a_tfrecord_cache(tmp_path):
    from yolo_tf_amd.utils import tfrecord
    path = str(tmp_path / 'train.tfrecord')
    tfrecord.write_cache(path, SAMPLES)          # the image files do not exist: nothing may open them
    objects, sizes = A.cache_objects([path])
    assert sizes == [(200, 100), (416, 416), (40, 50)]
    got = A.boxes_in_cells(objects, sizes, 13, 13)
    assert got.dtype == np.float32 and got.shape == (3, 2) and bits(got) == bits(WANT_13)
    assert bits(A.read_boxes('cache', 13, 13, cache_paths=[path])) == bits(WANT_13)
    wide = A.boxes_in_cells(objects, sizes, 19, 10)          # a non-square grid: x and y scale separately
    assert bits(wide) == bits(np.array([[9.5, 5], [19, 10], [32 / 416 * 19, 64 / 416 * 10]], np.float32))


def test_boxes_in_cells_from_an_npz(tmp_path):
    images = np.empty(3, object)
    for i, (_, shape, _, _) in enumerate(SAMPLES):
        images[i] = np.zeros(shape, np.uint8)
    cls = np.concatenate([np.asarray(s[2], np.int32) for s in SAMPLES])
    coord = np.concatenate([np.asarray(s[3], np.float32).reshape(-1, 4) for s in SAMPLES])
    path = str(tmp_path / 'data.npz')
    np.savez(path, images=images, objects_class=cls, objects_coord=coord, objects_first=np.array([0, 2, 3, 3]))
    assert bits(A.read_boxes(path, 13, 13)) == bits(WANT_13)


def test_non_positive_extents_and_out_of_range_values_raise():
    ok = [([0], [[1, 1, 5, 5]])]
    assert A.boxes_in_cells(ok, [(10, 10)], 13, 13).shape == (1, 2)
    for bad in ([[5, 1, 5, 9]], [[6, 1, 5, 9]], [[1, 9, 5, 2]], [[1, 1, np.nan, 5]], [[1, 1, np.inf, 5]]):
        with pytest.raises(ValueError):
            A.boxes_in_cells([([0], bad)], [(10, 10)], 13, 13)
    with pytest.raises(ValueError):
        A.boxes_in_cells(ok, [(0, 10)], 13, 13)
    assert A.validate_boxes([[2.0 ** -12, 4095.99]]).dtype == np.float32
    for bad in ([[2.0 ** -13, 1]], [[1, 4096]], [[1, -1]], [[0, 1]], [[np.nan, 1]], [[np.inf, 1]], np.zeros((0, 2)), [1, 2, 3], np.ones((4, 3))):
        with pytest.raises(ValueError):
            A.validate_boxes(bad)
    with pytest.raises(ValueError):
        A.initial_indices(3, [4], 0)


def test_initialisation_is_distinct_seeded_and_in_job_order():
    job_k, job_r = A.job_table([1, 3, 2], 2)
    assert job_k.tolist() == [1, 1, 3, 3, 2, 2] and job_r.tolist() == [0, 1, 0, 1, 0, 1]
    a, b = A.initial_indices(5, job_k, 7), A.initial_indices(5, job_k, 7)
    assert [x.tolist() for x in a] == [x.tolist() for x in b]
    assert all(len(set(x.tolist())) == len(x) == k and 0 <= x.min() and x.max() < 5 for x, k in zip(a, job_k))
    assert [x.tolist() for x in A.initial_indices(5, job_k, 8)] != [x.tolist() for x in a]
    assert sorted(A.initial_indices(3, [3], 0)[0].tolist()) == [0, 1, 2]


# ---------------------------------------------------------------- the anchor file
def test_write_anchors_round_trip_is_bitwise(tmp_path):
    rng = np.random.RandomState(6)
    a = np.exp(rng.normal(0, 3, (32, 2))).astype(np.float32)
    a[0] = [2.0 ** -12, np.nextafter(np.float32(4096), np.float32(0))]
    a[1] = [np.float32(1) / np.float32(3), np.float32(0.1)]
    path = str(tmp_path / 'anchors.tsv')
    A.write_anchors(path, a)
    with open(path) as f:
        lines = f.read().split('\n')
    assert lines[0] == 'w\th' and len(lines) == 34 and lines[-1] == '' and all(len(line.split('\t')) == 2 for line in lines[:-1])
    back = utils.read_anchors(path)
    assert back.dtype == np.float32 and bits(back) == bits(a)


def test_the_shipped_voc_anchors_round_trip(tmp_path):
    src = os.path.join(ROOT, 'config', 'yolo2', 'anchors', 'voc.tsv')
    a = utils.read_anchors(src)
    assert a.shape == (5, 2)
    path = str(tmp_path / 'voc.tsv')
    A.write_anchors(path, a)
    assert bits(utils.read_anchors(path)) == bits(a)
    assert open(path).read() == open(src).read()          # the shortest text of every value is the text that was shipped
    s, c = A.sort_by_area([[3, 3], [1, 1], [2, 2], [1, 1]], [30, 10, 20, 11])
    assert s[:, 0].tolist() == [1, 1, 2, 3] and c.tolist() == [10, 11, 20, 30]


# ---------------------------------------------------------------- command line
def test_cli_argument_rules():
    import anchors as cli          # the top-level tool: import-safe, nothing runs
    assert cli.parse_ks('5') == [5] and cli.parse_ks('1-16') == list(range(1, 17))
    a = cli.make_args(['-k', '5', '-o', 'x.tsv'])
    assert a.k == [5] and a.output == 'x.tsv' and a.restarts == 16 and a.max_iter == 500 and a.data == 'cache'
    a = cli.make_args(['-k', '1-16', '--data', 'synthetic', '--boxes', '1000', '--json', 's.json'])
    assert a.k == list(range(1, 17)) and a.output is None and a.pick is None
    a = cli.make_args(['-k', '1-6', '--pick', '5', '-o', 'x.tsv'])
    assert a.pick == 5
    assert cli.make_args(['--score', 'config/yolo2/anchors/voc.tsv']).score
    for bad in (['-k', '5'], ['-k', '1-6', '--pick', '7', '-o', 'x.tsv'], ['-k', '1-6', '--pick', '5'], ['-k', '0', '-o', 'x'], ['-k', '3-2', '-o', 'x'],
                ['-k', '1-33', '-o', 'x'], ['-k', 'five', '-o', 'x']):
        with pytest.raises(SystemExit):
            cli.make_args(bad)


# ---------------------------------------------------------------- C ABI: argument errors come back before any launch
def test_anchor_abi_argument_errors_raise_without_touching_the_gpu():
    from yolo_tf_amd import _lib
    q = _lib.query
    assert q('yolo2_anchor_workspace_bytes', 1, 1) == 8 * 4 and q('yolo2_anchor_workspace_bytes', 256, 16) == 8 * 256 * 49
    assert q('yolo2_anchor_workspace_bytes', 3, 32) == 8 * 3 * 97
    assert q('yolo2_anchor_workspace_bytes', 0, 5) == 0 and q('yolo2_anchor_workspace_bytes', 1, 33) == 0
    P = 4096          # a non-null, aligned value standing in for device pointers: an argument error returns before anything reads it
    ok_assign = [P, 10, P, P, 2, 5, P, 8 * 2 * 16, None, None, None]
    ok_update = [P, P, 2, 5, P, 8 * 2 * 16, 10, P, P, None, None, None]

    def bad(name, base, **changes):
        args = list(base)
        for i, v in changes.items():
            args[int(i[1:])] = v
        with pytest.raises(_lib.HipKernelError, match='argument check failed'):
            _lib.call(name, *args)
    for i in (0, 2, 3, 6):                                   # boxes, centroids, job_k, ws
        bad('yolo2_anchor_assign', ok_assign, **{'a%d' % i: None})
    bad('yolo2_anchor_assign', ok_assign, a0=P + 8)          # boxes: 16-byte loads
    for n in (0, -1, 1 << 27):
        bad('yolo2_anchor_assign', ok_assign, a1=n)
        bad('yolo2_anchor_update', ok_update, a6=n)
    for kmax in (0, 33):
        bad('yolo2_anchor_assign', ok_assign, a5=kmax, a7=1 << 20)
        bad('yolo2_anchor_update', ok_update, a3=kmax, a5=1 << 20)
    for jobs in (0, 65536):
        bad('yolo2_anchor_assign', ok_assign, a4=jobs, a7=1 << 30)
        bad('yolo2_anchor_update', ok_update, a2=jobs, a5=1 << 30)
    bad('yolo2_anchor_assign', ok_assign, a7=8 * 2 * 16 - 1)          # workspace one byte short
    bad('yolo2_anchor_update', ok_update, a5=8 * 2 * 16 - 1)
    for i in (0, 1, 4):                                      # centroids (update pass), job_k, ws
        bad('yolo2_anchor_update', ok_update, **{'a%d' % i: None})
    bad('yolo2_anchor_update', ok_update, a7=None)           # done without iterations
    bad('yolo2_anchor_update', ok_update, a8=None)
    bad('yolo2_anchor_update', ok_update, a7=None, a8=None)  # score pass without an output
