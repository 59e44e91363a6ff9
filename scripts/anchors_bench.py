"""Cost of the dimension-cluster sweep at the size a user runs (profiles/anchors.md; bench.py is the flagship benchmark and does not cover
this): 2^20 seeded synthetic boxes, k = 1 .. 16, 16 restarts = 256 jobs in every launch.

  1. whole-sweep wall time of DimensionClusters.fit, ending in a device synchronise, after a warm-up fit of the same sweep;
  2. the assign and update kernels' times from a `rocprofv3 --kernel-trace` run of its own (a fresh child process runs ONE sweep under
     the profiler; tracing slows the host, so the wall time of that run is not used);
  3. box-centroid pairs per second: pairs = sum over jobs of (updates applied + the score pass) x k x N;
  4. the NumPy specification (tests/anchors_ref.py) for ONE iteration of one k = 16 job on the same box's CPU, and the host time of the
     whole sweep EXTRAPOLATED from it by pairs (labelled as such: nobody ran the sweep on the host).

Prints one JSON line; ``--markdown FILE`` also writes the record for profiles/anchors.md.  No pass / fail threshold: there is no earlier
number to compare with."""
import argparse
import csv
import glob
import json
import os
import platform
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def sweep(args):
    """One fit of the whole sweep: (result, raw job table, wall seconds including the final synchronise)."""
    import torch
    from yolo_tf_amd import anchors
    boxes = anchors.synthetic_boxes(args.boxes, 13, 13, seed=args.seed)
    dc = anchors.DimensionClusters(boxes)
    ks = list(range(1, args.kmax + 1))
    times = []
    for _ in range(1 if args.sweep_only else 1 + args.reps):          # the first one is the warm-up (code objects, allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = dc.fit(ks, restarts=args.restarts, max_iter=args.max_iter, seed=args.seed)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return boxes, result, dc.last_jobs, times


def pairs_of(jobs, n):
    """Box-centroid pairs the sweep evaluated: every update applied and the score pass, k x N each."""
    return int(sum((int(it) + 1) * int(k) * n for it, k in zip(jobs['iterations'], jobs['job_k'])))


def kernel_times(trace_dir):
    """{kernel: (calls, total ms, longest ms)} of the two anchor kernels from a rocprofv3 --kernel-trace CSV."""
    agg = {}
    for f in glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True):
        for r in csv.DictReader(open(f)):
            for name in ('anchor_assign_kernel', 'anchor_update_kernel'):
                if name in r['Kernel_Name']:
                    ms = (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6
                    a = agg.setdefault(name, [0, 0.0, 0.0])
                    a[0] += 1
                    a[1] += ms
                    a[2] = max(a[2], ms)
    return agg


def profile(args):
    """Runs `--sweep-only` in a fresh child process under rocprofv3 and reads its kernel trace."""
    out_dir = args.trace_dir or tempfile.mkdtemp(prefix='anchors_prof_')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '-o', 'anchors', '--', sys.executable,
           os.path.abspath(__file__), '--sweep-only', '--boxes', str(args.boxes), '--kmax', str(args.kmax), '--restarts', str(args.restarts),
           '--max_iter', str(args.max_iter), '--seed', str(args.seed)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.profile_timeout)
    if r.returncode != 0:
        raise RuntimeError('rocprofv3 run failed (%d)\n%s\n%s' % (r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    agg = kernel_times(out_dir)
    if 'anchor_assign_kernel' not in agg:
        raise RuntimeError('no anchor kernels in the trace under %s' % out_dir)
    child = json.loads([line for line in r.stdout.splitlines() if line.startswith('{')][-1])
    return agg, child


def cpu_reference(boxes, n_cpu):
    """Seconds of ONE specification iteration (assign + sums + update) of a k = 16 job on the host, and the pairs it evaluated."""
    import anchors_ref as R
    from yolo_tf_amd import anchors
    b = boxes[:n_cpu]
    cen = b[anchors.initial_indices(len(b), [16], 0)[0]]
    R.step(b[:4096], cen)
    t0 = time.perf_counter()
    R.step(b, cen)
    return time.perf_counter() - t0, 16 * len(b)


def main(args):
    import numpy as np
    import torch
    boxes, result, jobs, times = sweep(args)
    n = len(boxes)
    pairs = pairs_of(jobs, n)
    out = {'device': torch.cuda.get_device_name(0), 'host': platform.node(), 'boxes': n, 'ks': [1, args.kmax], 'restarts': args.restarts,
           'jobs': len(jobs['job_k']), 'pairs': pairs, 'launch_pairs': int(jobs['iterations'].max()) + 1,
           'iterations_min_median_max': [int(jobs['iterations'].min()), float(np.median(jobs['iterations'])), int(jobs['iterations'].max())],
           'converged_jobs': int(jobs['converged'].sum()),
           'avg_iou_by_k': {str(k): result[k]['avg_iou'] for k in sorted(result)}}
    if args.sweep_only:
        out['sweep_s_under_profiler'] = times[0]
        print(json.dumps(out))
        return
    timed = times[1:]
    out.update(warmup_sweep_s=times[0], sweep_s=float(np.median(timed)), sweep_s_all=timed)
    out['pairs_per_s_whole_sweep'] = pairs / out['sweep_s']
    if not args.no_profile:
        agg, child = profile(args)
        assert child['pairs'] == pairs, 'the profiled sweep is not the timed one'
        out['kernels'] = {name: {'calls': c, 'total_ms': t, 'mean_ms': t / c, 'longest_ms': longest} for name, (c, t, longest) in agg.items()}
        out['pairs_per_s_assign_kernel'] = pairs / (agg['anchor_assign_kernel'][1] / 1e3)
        # atomics of the assign kernel at full load (the longest launch: every job active): at most 3 k + 1 words of 8 bytes per workgroup
        chunks = (n + 4095) // 4096
        out['atomic_bytes_full_launch_upper_bound'] = int(sum(8 * (3 * int(k) + 1) * chunks for k in jobs['job_k']))
    sec, cpu_pairs = cpu_reference(boxes, min(n, args.cpu_boxes))
    out['cpu_reference'] = {'boxes': min(n, args.cpu_boxes), 'k': 16, 'one_iteration_s': sec, 'pairs_per_s': cpu_pairs / sec,
                            'host_sweep_s_EXTRAPOLATED': pairs / (cpu_pairs / sec)}
    print(json.dumps(out))
    if args.markdown:
        with open(args.markdown, 'w') as f:
            f.write(markdown(out))


def markdown(o):
    lines = ['Measured by `scripts/anchors_bench.py` on `%s` (host `%s`).' % (o['device'], o['host']), '',
             '| quantity | value |', '|---|---:|',
             '| boxes (seeded synthetic, 13 x 13 grid) | %d |' % o['boxes'],
             '| jobs per launch (k = %d .. %d x %d restarts) | %d |' % (o['ks'][0], o['ks'][1], o['restarts'], o['jobs']),
             '| assign + update pairs the longest job needed (its updates + the score pass) | %d |' % o['launch_pairs'],
             '| updates per job: min / median / max | %d / %.0f / %d |' % tuple(o['iterations_min_median_max']),
             '| jobs at their fixed point | %d of %d |' % (o['converged_jobs'], o['jobs']),
             '| box-centroid pairs evaluated | %.4g |' % o['pairs'],
             '| whole sweep, wall, final synchronise included, after a warm-up sweep (median of %d) | %.3f s |' % (len(o['sweep_s_all']), o['sweep_s']),
             '| the warm-up sweep itself | %.3f s |' % o['warmup_sweep_s'],
             '| pairs per second over the whole sweep (wall) | %.4g |' % o['pairs_per_s_whole_sweep']]
    for name, k in sorted(o.get('kernels', {}).items()):
        lines.append('| `%s` (rocprofv3 --kernel-trace, a run of its own): launches / total / mean / longest | %d / %.2f ms / %.4f ms / %.4f ms |'
                     % (name, k['calls'], k['total_ms'], k['mean_ms'], k['longest_ms']))
    if 'kernels' in o:
        lines.append('| pairs per second inside the assign kernel | %.4g |' % o['pairs_per_s_assign_kernel'])
        lines.append('| global atomic bytes of one full-load assign launch (upper bound: every table word non-zero) | %.3g MB |'
                     % (o['atomic_bytes_full_launch_upper_bound'] / 1e6))
    c = o['cpu_reference']
    lines += ['| NumPy specification, ONE iteration of one k = 16 job at %d boxes, the same box\'s CPU | %.3f s (%.3g pairs/s) |'
              % (c['boxes'], c['one_iteration_s'], c['pairs_per_s']),
              '| the whole sweep on the host, EXTRAPOLATED from that by pairs (never run) | %.0f s |' % c['host_sweep_s_EXTRAPOLATED'], '',
              'Best average IoU by k: ' + ', '.join('%s: %.4f' % (k, v) for k, v in sorted(o['avg_iou_by_k'].items(), key=lambda kv: int(kv[0]))), '']
    return '\n'.join(lines)


if __name__ == '__main__':
    p = argparse.ArgumentParser()
    p.add_argument('--boxes', type=int, default=1 << 20)
    p.add_argument('--kmax', type=int, default=16, help='the sweep is k = 1 .. kmax')
    p.add_argument('--restarts', type=int, default=16)
    p.add_argument('--max_iter', type=int, default=500)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--reps', type=int, default=3, help='timed sweeps after the warm-up')
    p.add_argument('--cpu_boxes', type=int, default=1 << 20, help='boxes of the host iteration')
    p.add_argument('--sweep-only', dest='sweep_only', action='store_true', help='one sweep, no warm-up, no profile, no host reference (the profiled child)')
    p.add_argument('--no_profile', action='store_true')
    p.add_argument('--trace_dir', help='where rocprofv3 writes (default: a temporary directory)')
    p.add_argument('--profile_timeout', type=float, default=300)
    p.add_argument('--markdown')
    main(p.parse_args())
