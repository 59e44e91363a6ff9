"""What a training step and a detection launch, as a list: every call of a function of ``yolo_tf_amd.ops`` that is handed a device buffer, as
[name, stream ('m' main / 's' side), arguments ..., {keyword arguments, if any}]; a tensor argument is its dtype letter (DTYPES) followed by its
element count, e.g. "b*147456".  Host queries (no tensor argument) are left out: when the engine asks them is not part of what it launches.

tests/test_engine_launches_gpu.py compares these lists with tests/golden/engine_launches.json.gz (gzip of one JSON document, one call per line:
``zcat`` shows it);

    python tests/engine_launch_log.py --out tests/golden/engine_launches.json.gz

records that file on a GPU (one pass per network and dtype, in this process)."""
import gzip
import io
import json
import os
import subprocess
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BATCH, SIZE, CLASSES = 2, 96, 20         # 96: the smallest size with an even 26 -> 13-style passthrough grid (6 -> 3)
DTYPES = {'float32': 'f', 'bfloat16': 'b', 'float64': 'd', 'uint8': 'u', 'int32': 'i', 'int64': 'l'}
SCENARIOS = [(net, dtype) for net in ('darknet', 'tiny') for dtype in ('bf16', 'f32')]


class Recorder(object):
    """``with Recorder() as log:`` replaces every public function of the ops module with a logging wrapper for the duration of the block."""

    def __enter__(self):
        import torch
        from yolo_tf_amd import ops
        self.ops, self.saved, self.log = ops, {}, []
        main = torch.cuda.current_stream().cuda_stream

        def enc(a, seen):
            if isinstance(a, torch.Tensor):
                seen.append(a)
                return '%s*%d' % (DTYPES[str(a.dtype).replace('torch.', '')], a.numel())
            if a is None or isinstance(a, (bool, int, float, str)):
                return a
            if isinstance(a, (list, tuple)):
                return [enc(x, seen) for x in a]
            return str(a) if isinstance(a, torch.dtype) else type(a).__name__

        def wrap(name, fn):
            def logged(*args, **kwargs):
                seen = []
                entry = [name, 'm' if torch.cuda.current_stream().cuda_stream == main else 's'] + enc(args, seen)
                if kwargs:
                    entry.append({k: enc(v, seen) for k, v in sorted(kwargs.items())})
                if seen:
                    self.log.append(entry)
                return fn(*args, **kwargs)
            return logged
        for name, fn in vars(ops).items():
            if isinstance(fn, types.FunctionType) and fn.__module__ == ops.__name__ and not name.startswith('_'):
                self.saved[name] = fn
        for name, fn in self.saved.items():
            setattr(ops, name, wrap(name, fn))
        return self.log

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.ops, name, fn)
        return False


def inputs(batch, size, cells):
    import numpy as np
    import torch
    from yolo_tf_amd.utils import data
    images = np.random.RandomState(0).uniform(0, 255, (batch, size, size, 3)).astype(np.float32)
    return torch.from_numpy(images).cuda(), data.synthetic_batch(batch, CLASSES, cells, cells, seed=2)


def record(net, dtype, batch=BATCH, size=SIZE, **session_args):
    """-> {'train': the first training step of a fresh session, 'infer': the first detection of a fresh session}"""
    import torch
    from bench import make_builder
    from yolo_tf_amd.session import DetectSession, TrainSession
    out = {}
    images, labels = inputs(batch, size, size // 32)
    builder, _ = make_builder(net, CLASSES, size, True, tempfile.mkdtemp(prefix='launch_log_'))
    sess = TrainSession(builder, batch, dtype=dtype, optimizer='adam', learning_rate=1e-3, seed=1, **session_args)
    with Recorder() as log:
        sess.step(images, labels)
        sess.fetch()
    out['train'] = log
    builder, _ = make_builder(net, CLASSES, size, False, tempfile.mkdtemp(prefix='launch_log_'))
    det = DetectSession(builder, batch, dtype=dtype, seed=1)
    with Recorder() as log:
        det.run(images, check_numerics=False)       # (untrained weights: exp() of a raw logit may overflow, which is not what is recorded)
        torch.cuda.synchronize()
    out['infer'] = log
    return json.loads(json.dumps(out))          # (tuples -> lists, as a stored log reads back)


def read(path):
    with gzip.open(path, 'rt') as f:
        return json.load(f)


def write(path, commit, logs):
    with open(path, 'wb') as raw, gzip.GzipFile(filename='', mode='wb', fileobj=raw, mtime=0) as z, io.TextIOWrapper(z) as f:       # (mtime 0: same bytes every time)
        f.write('{\n "commit": %s,\n "batch": %d, "size": %d,\n "dtypes": %s,\n "logs": {\n' % (json.dumps(commit), BATCH, SIZE, json.dumps(DTYPES)))
        parts = []
        for key, log in logs.items():
            for phase in ('train', 'infer'):
                parts.append('  %s: [\n' % json.dumps('%s %s' % (key, phase)) + ',\n'.join('   ' + json.dumps(e, separators=(',', ':')) for e in log[phase]) + '\n  ]')
        f.write(',\n'.join(parts))
        f.write('\n }\n}\n')


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'engine_launches.json.gz'))
    ap.add_argument('--commit', default=None, help='the commit whose launches these are (default: the checkout\'s HEAD)')
    args = ap.parse_args()
    commit = args.commit or subprocess.run(['git', '-C', ROOT, 'rev-parse', 'HEAD'], capture_output=True, text=True).stdout.strip() or 'unknown'
    logs = {'%s %s' % (net, dtype): record(net, dtype) for net, dtype in SCENARIOS}
    write(args.out, commit, logs)
    print('wrote %s: %s' % (args.out, ', '.join('%s %d+%d' % (k, len(v['train']), len(v['infer'])) for k, v in logs.items())))
    return 0


if __name__ == '__main__':
    sys.exit(main())
