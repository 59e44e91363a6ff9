"""Dimension clusters on the device against the NumPy specification (tests/anchors_ref.py).  Every comparison is exact: integer equality,
f32 bit patterns, f64 ==.  Inputs are seeded."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anchors_ref as R  # noqa: E402

from yolo_tf_amd import anchors as A  # noqa: E402
from yolo_tf_amd import utils  # noqa: E402

SENTINEL = np.float32(777.25)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).tolist()


def lognormal(n, seed):
    return np.exp(np.random.RandomState(seed).normal(1.0, 0.6, (n, 2))).astype(np.float32)


def device_step(boxes, job_k, cen, frozen=()):
    """One yolo2_anchor_assign + yolo2_anchor_update through the raw wrappers: everything the two entries write, on the host."""
    import torch

    from yolo_tf_amd import ops
    J, kmax, n = len(job_k), cen.shape[1], len(boxes)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_boxes, d_cen, d_k = t(boxes), t(cen), t(np.asarray(job_k, np.int32))
    ws = torch.zeros(J * (3 * kmax + 1), dtype=torch.int64, device='cuda')
    done = torch.zeros(J, dtype=torch.int32, device='cuda')
    for j in frozen:
        done[j] = 1
    iterations = torch.zeros(J, dtype=torch.int32, device='cuda')
    counts = torch.full((J, kmax), -7, dtype=torch.int64, device='cuda')
    avg = torch.full((J,), -7.0, dtype=torch.float64, device='cuda')
    assignment = torch.full((J, n), 255, dtype=torch.uint8, device='cuda')
    ops.anchor_assign(d_boxes, n, d_cen, d_k, J, kmax, ws, done=done, assignment=assignment)
    ops.anchor_update(d_cen, d_k, J, kmax, ws, n, done=done, iterations=iterations, counts=counts, avg_iou=avg)
    torch.cuda.synchronize()
    return dict(centroids=d_cen.cpu().numpy(), done=done.cpu().numpy(), iterations=iterations.cpu().numpy(), counts=counts.cpu().numpy(),
                avg_iou=avg.cpu().numpy(), assignment=assignment.cpu().numpy(), ws=ws.cpu().numpy())


def check_step(got, j, boxes, cen, k):
    """Job j of a device_step against one reference step from the centroids cen[:k]."""
    new, count, avg, arg = R.step(boxes, cen[:k])
    assert bits(got['centroids'][j, :k]) == bits(new)
    assert bits(got['centroids'][j, k:]) == bits(cen[k:])                     # slots past k: untouched
    assert got['counts'][j, :k].tolist() == count.tolist() and (got['counts'][j, k:] == -7).all()
    assert got['avg_iou'][j] == avg
    assert (got['assignment'][j] == arg).all()
    assert got['iterations'][j] == 1 and got['done'][j] == int(bits(new) == bits(cen[:k]))
    assert not got['ws'].any()                                                 # the update cleared what the assign added
    return new, count


# ---------------------------------------------------------------- single iteration
@pytest.mark.parametrize('k', [1, 2, 5, 16, 32])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 4099])          # wave, workgroup (256 lanes) and chunk (4096 boxes) tails, odd and even
def test_one_iteration_matches_the_specification(n, k):
    boxes = lognormal(n, 100 + n)
    cen = np.full((1, 32, 2), SENTINEL, np.float32)                  # kmax = 32: full at k = 32, nearly empty at k = 1
    cen[0, :k] = lognormal(k, 200 + k)
    got = device_step(boxes, [k], cen)
    check_step(got, 0, boxes, cen[0], k)


# ---------------------------------------------------------------- ties and empty clusters
def test_ties_go_to_the_lowest_index_and_empty_clusters_keep_their_bits():
    g = np.arange(1, 9, dtype=np.float32) * np.float32(0.5)
    boxes = np.stack(np.meshgrid(g, g, indexing='ij'), -1).reshape(-1, 2)          # w, h in {0.5, ..., 4}: 64 boxes
    cen = np.array([[1, 2], [2, 1], [1, 2], [2, 2], [2, 1], [4, 4], [8, 8], [2, 2]], np.float32)      # 2 = 0, 4 = 1, 7 = 3; (1,1) ties 0 with 1
    got = device_step(boxes, [8], cen[None].copy())
    new, count = check_step(got, 0, boxes, cen, 8)
    arg = got['assignment'][0]
    assert arg[list(map(tuple, boxes)).index((1.0, 1.0))] == 0                     # IoU 0.5 with (1,2) and with (2,1)
    assert not np.isin(arg, [2, 4, 7]).any() and count[[2, 4, 7]].tolist() == [0, 0, 0]
    assert bits(got['centroids'][0][[2, 4, 7]]) == bits(cen[[2, 4, 7]])
    assert count[6] == 0 and bits(got['centroids'][0][6]) == bits(cen[6])           # (8,8): IoU at most 1/4, (4,4) is never worse


# ---------------------------------------------------------------- many jobs in one launch
def test_every_job_of_a_launch_equals_the_job_alone_and_the_specification():
    boxes = lognormal(513, 7)
    dc = A.DimensionClusters(boxes)
    job_k, _ = A.job_table(range(1, 9), 3)
    cen = np.full((len(job_k), 8, 2), SENTINEL, np.float32)
    for j, idx in enumerate(A.initial_indices(len(boxes), job_k, 11)):
        cen[j, :len(idx)] = boxes[idx]
    together = dc.run_jobs(job_k, cen, max_iter=4, check_every=2)
    for j, k in enumerate(job_k):
        alone = dc.run_jobs(job_k[j:j + 1], cen[j:j + 1], max_iter=4, check_every=4)
        want, it, conv = R.fit(boxes, cen[j, :k], 4)
        for r, i in ((together, j), (alone, 0)):
            assert bits(r['centroids'][i, :k]) == bits(want) and bits(r['centroids'][i, k:]) == bits(cen[j, k:])
            assert r['iterations'][i] == it and r['converged'][i] == conv
            avg, count, _ = R.score(boxes, want)
            assert r['avg_iou'][i] == avg and r['counts'][i, :k].tolist() == count.tolist() and (r['counts'][i, k:] == -1).all()


def test_a_frozen_job_is_left_alone():
    boxes = lognormal(300, 8)
    cen = np.stack([lognormal(4, 9), lognormal(4, 10)])
    got = device_step(boxes, [4, 3], cen, frozen=(0,))
    assert bits(got['centroids'][0]) == bits(cen[0]) and got['iterations'][0] == 0 and got['done'][0] == 1
    assert (got['counts'][0] == -7).all() and got['avg_iou'][0] == -7.0 and (got['assignment'][0] == 255).all()
    check_step(got, 1, boxes, cen[1], 3)


# ---------------------------------------------------------------- many workgroups per job, run to run
def test_many_workgroups_add_into_the_same_sums_reproducibly():
    boxes = lognormal(65537, 12)                                     # 17 workgroups per job, the last one with a single box
    cen = boxes[A.initial_indices(len(boxes), [9], 13)[0]][None]
    runs = {}
    for max_iter in (1, 5):
        want, it, conv = R.fit(boxes, cen[0], max_iter)
        avg, count, arg = R.score(boxes, want)
        for fresh in range(2):                                       # fresh buffers each time, as two processes would have
            dc = A.DimensionClusters(boxes)
            for again in range(2):
                r = dc.run_jobs([9], cen, max_iter=max_iter, assignments=(0,))
                runs.setdefault(max_iter, []).append(r)
                assert bits(r['centroids'][0]) == bits(want) and r['iterations'][0] == it and r['converged'][0] == conv
                assert r['avg_iou'][0] == avg and r['counts'][0].tolist() == count.tolist() and (r['assignments'][0] == arg).all()
    for rs in runs.values():
        assert all(bits(r['centroids']) == bits(rs[0]['centroids']) and r['avg_iou'][0] == rs[0]['avg_iou'][0] for r in rs)


# ---------------------------------------------------------------- sums beyond 2^53
def test_fixed_point_sums_beyond_2_to_the_53():
    rng = np.random.RandomState(14)
    boxes = rng.uniform(3900, 4095, (262144, 2)).astype(np.float32)
    cen = np.array([[[3950, 3950], [4050, 4050]]], np.float32)
    arg, best = R.assign(boxes, cen[0])
    count, sw, sh, _ = R.sums(boxes, arg, best, 2)
    assert min(int(sw.max()), int(sh.max())) > 1 << 53          # the case is what it says: a cluster's sums are past the integers f64 holds exactly
    got = device_step(boxes, [2], cen.copy())
    check_step(got, 0, boxes, cen[0], 2)
    r = A.DimensionClusters(boxes).run_jobs([2], cen, max_iter=3)
    want, it, conv = R.fit(boxes, cen[0], 3)
    assert bits(r['centroids'][0]) == bits(want) and r['iterations'][0] == it and r['converged'][0] == conv
    assert r['avg_iou'][0] == R.score(boxes, want)[0]


def test_smallest_and_largest_extents_in_one_job():
    rng = np.random.RandomState(15)
    tiny = np.full((500, 2), 2.0 ** -12, np.float32)
    tiny[1::2] *= rng.uniform(1, 4, (250, 2)).astype(np.float32)
    huge = rng.uniform(2000, 4095.9, (501, 2)).astype(np.float32)
    huge[0] = np.nextafter(np.float32(4096), np.float32(0))
    boxes = np.concatenate([tiny, huge])[rng.permutation(1001)]
    cen = np.array([[[2.0 ** -12, 2.0 ** -12], [4000, 4000], [1, 1], [2.0 ** -11, 2.0 ** -12]]], np.float32)
    got = device_step(boxes, [4], cen.copy())
    check_step(got, 0, boxes, cen[0], 4)


# ---------------------------------------------------------------- fit to a fixed point, and the cut-off
FIT_KS, FIT_RESTARTS, FIT_SEED = (5, 16), 4, 21


@functools.lru_cache(maxsize=None)
def fit_case(max_iter):
    """(boxes, job_k, initial centroids, the specification's (centroids, iterations, converged, avg_iou, counts) per job): computed once."""
    boxes = lognormal(4099, 20)
    job_k, _ = A.job_table(FIT_KS, FIT_RESTARTS)
    init = [boxes[idx] for idx in A.initial_indices(len(boxes), job_k, FIT_SEED)]
    want = []
    for c in init:
        cen, it, conv = R.fit(boxes, c, max_iter)
        avg, count, _ = R.score(boxes, cen)
        want.append((cen, it, conv, avg, count))
    return boxes, job_k, init, want


def check_fit(result, jobs, boxes, want):
    for i, k in enumerate(FIT_KS):
        per_job = want[i * FIT_RESTARTS:(i + 1) * FIT_RESTARTS]
        for r, (cen, it, conv, avg, count) in enumerate(per_job):
            j = i * FIT_RESTARTS + r
            assert bits(jobs['centroids'][j, :k]) == bits(cen) and jobs['iterations'][j] == it and jobs['converged'][j] == conv
            assert jobs['avg_iou'][j] == avg and jobs['counts'][j, :k].tolist() == count.tolist()
        avgs = [w[3] for w in per_job]
        best = int(np.argmax(avgs))
        cen, it, conv, avg, count = per_job[best]
        anchors, counts = A.sort_by_area(cen, count)
        got = result[k]
        assert got['restart'] == best and got['restart_avg_iou'] == avgs and got['avg_iou'] == avg
        assert bits(got['anchors']) == bits(anchors) and got['counts'].tolist() == counts.tolist()
        assert got['iterations'] == it and got['converged'] == conv
        areas = got['anchors'][:, 0].astype(np.float64) * got['anchors'][:, 1]
        assert (np.diff(areas) >= 0).all()


@pytest.mark.parametrize('check_every', [1, 7])
def test_fit_runs_every_job_to_its_fixed_point(check_every):
    boxes, job_k, init, want = fit_case(500)
    assert all(w[2] and w[1] < 500 for w in want)                    # max_iter = 500 is no cap any job runs into
    dc = A.DimensionClusters(boxes)
    result = dc.fit(FIT_KS, restarts=FIT_RESTARTS, max_iter=500, seed=FIT_SEED, check_every=check_every)
    check_fit(result, dc.last_jobs, boxes, want)


def test_cut_off_jobs_report_the_state_after_max_iter_updates():
    boxes, job_k, init, want = fit_case(3)
    assert not any(w[2] for w in want) and all(w[1] == 3 for w in want)
    dc = A.DimensionClusters(boxes)
    result = dc.fit(FIT_KS, restarts=FIT_RESTARTS, max_iter=3, seed=FIT_SEED)
    check_fit(result, dc.last_jobs, boxes, want)
    for k in FIT_KS:                                                 # the reported average IoU belongs to the returned centroids
        avg, counts = dc.score(result[k]['anchors'])
        assert avg == R.score(boxes, result[k]['anchors'])[0]
        assert sorted(counts.tolist()) == sorted(result[k]['counts'].tolist())
    with pytest.raises(ValueError):
        A.DimensionClusters(boxes[:4]).fit([5])                      # k > N


# ---------------------------------------------------------------- score
def test_score_of_the_shipped_voc_anchors():
    boxes = A.synthetic_boxes(3001, 13, 13, seed=30)
    voc = utils.read_anchors(os.path.join(ROOT, 'config', 'yolo2', 'anchors', 'voc.tsv'))
    avg, counts, arg = A.DimensionClusters(boxes).score(voc, assignment=True)
    want_avg, want_counts, want_arg = R.score(boxes, voc)
    assert avg == want_avg and counts.tolist() == want_counts.tolist() and (arg == want_arg).all() and arg.dtype == np.uint8
    assert 0.3 < avg < 1.0 and counts.sum() == 3001


# ---------------------------------------------------------------- the tool as a user runs it
def test_cli_end_to_end(tmp_path):
    overlay = tmp_path / 'local.ini'
    overlay.write_text('[config]\nbasedir = %s\n' % tmp_path)
    tsv, out_json = tmp_path / 'my_anchors.tsv', tmp_path / 'sweep.json'
    cmd = [sys.executable, 'anchors.py', '-c', 'config.ini', 'config/yolo2/darknet-20.ini', str(overlay), '--data', 'synthetic', '--boxes', '5000',
           '-k', '1-6', '--restarts', '4', '--pick', '5', '-o', str(tsv), '--json', str(out_json)]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, 'FAILED: %s\n--- stdout\n%s\n--- stderr\n%s' % (' '.join(cmd), r.stdout[-3000:], r.stderr[-3000:])
    rows = [line.split() for line in r.stdout.splitlines() if line.split() and line.split()[0].isdigit()]
    assert [int(row[0]) for row in rows] == [1, 2, 3, 4, 5, 6]
    got = utils.read_anchors(str(tsv))
    assert got.shape == (5, 2) and (np.diff(got[:, 0].astype(np.float64) * got[:, 1]) >= 0).all()
    fit = A.DimensionClusters(A.synthetic_boxes(5000, 13, 13, seed=0)).fit(range(1, 7), restarts=4, seed=0)
    assert bits(got) == bits(fit[5]['anchors'])
    sweep = json.loads(out_json.read_text())
    assert sweep['boxes'] == 5000 and sweep['cells'] == [13, 13] and [s['k'] for s in sweep['sweep']] == [1, 2, 3, 4, 5, 6]
    for s in sweep['sweep']:
        assert s['avg_iou'] == fit[s['k']]['avg_iou'] and bits(s['anchors']) == bits(fit[s['k']]['anchors']) and s['converged']
        assert float(rows[s['k'] - 1][1]) == round(s['avg_iou'], 6)
    avgs = [s['avg_iou'] for s in sweep['sweep']]
    assert avgs[0] < avgs[2] < avgs[5]                                # more anchors fit better (the paper's figure)
    # a model configured with the fitted anchors builds
    from yolo_tf_amd.model import yolo2
    cfg = utils.make_config([os.path.join(ROOT, 'config.ini'), os.path.join(ROOT, 'config', 'yolo2', 'darknet-20.ini')], str(tmp_path))
    cfg.set('cache', 'names', os.path.join(ROOT, cfg.get('cache', 'names')))
    cfg.set('yolo2', 'anchors', str(tsv))
    utils.ensure_names(cfg)
    builder = yolo2.Builder(None, cfg)
    builder(None)
    assert bits(builder.anchors) == bits(got) and len(builder.model.anchors) == 5
