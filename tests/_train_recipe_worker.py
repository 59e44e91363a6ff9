"""One rank of tests/test_train_recipe_session_gpu.py::test_two_ranks_on_one_gpu: gradient accumulation (K = 2) with weight decay, data parallel over gloo
on the one GPU of the test box.  Every step that can wait for a peer runs under a time limit of its own."""
import os
import sys
import threading

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 2
UPDATES = 2


class limit(object):
    """A time limit around one step of a worker: a step that hangs (a collective whose peer is gone) ends the process."""

    def __init__(self, seconds, what):
        self.timer = threading.Timer(seconds, self._expire)
        self.timer.daemon = True
        self.what = what

    def _expire(self):
        sys.stderr.write('time limit: %s\n' % self.what)
        sys.stderr.flush()
        os._exit(124)

    def __enter__(self):
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()


def worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0')
    import torch.distributed as dist
    from test_network_gpu import make_builder
    from yolo_tf_amd.parallel import init_distributed
    from yolo_tf_amd.session import TrainSession
    from yolo_tf_amd.utils import data
    torch.cuda.set_device(0)
    with limit(120, 'process group'):
        init_distributed(backend='gloo')                # both ranks share the one GPU of the test box: gloo carries the CUDA tensors
    b, _ = make_builder('tiny', 20, 96, True, os.path.join(outdir, 'base%d' % rank))
    out = {}
    for tag, clip in (('deferred', 0.0), ('clip', 5.0)):          # the bucketed update as the buckets arrive, and the path that waits for all of them
        with limit(120, tag + ': session'):
            sess = TrainSession(b, 2, dtype='f32', optimizer='adam', learning_rate=1e-3, gradient_clip=clip, seed=3, world_size=world, bucket_mb=8.0,
                                accum_steps=K, weight_decay=5e-4)
            assert len(sess.reducer.buckets) >= 3 and sess.grad_acc is not None
            torch.cuda.synchronize()
        begun, launched = [], []
        begin, launch = sess.reducer.begin, sess.reducer._launch
        sess.reducer.begin = lambda: (begun.append((sess.global_step, sess.micro_step)), begin())[1]
        sess.reducer._launch = lambda s, e: (launched.append((sess.global_step, sess.micro_step)), launch(s, e))[1]
        e = sess.engine
        w0 = e.params.clone()
        for i in range(K * UPDATES):
            rng = np.random.RandomState(100 + 10 * i + rank)        # different data per rank and micro-batch, same initial weights (same seed)
            images = torch.from_numpy(rng.uniform(0, 255, (2, 96, 96, 3)).astype(np.float32)).cuda()
            with limit(120, '%s: micro-batch %d' % (tag, i)):
                sess.step(images, data.synthetic_batch(2, 20, 3, 3, seed=200 + 10 * i + rank))
                torch.cuda.synchronize()
            assert sess.micro_step == (i + 1) % K and sess.global_step == (i + 1) // K
            if i == 0:
                assert torch.equal(e.params, w0)                    # nothing was updated, nothing was exchanged
        out[tag + '/params'] = e.params.cpu().numpy()
        out[tag + '/slot0'] = sess.optimizer.slots[0].cpu().numpy()
        out[tag + '/w0'] = w0.cpu().numpy()
        out[tag + '/begun'] = np.array(begun, np.int64)
        out[tag + '/launched'] = np.array(launched, np.int64)
        out[tag + '/buckets'] = np.int64(len(sess.reducer.buckets))
    np.savez(os.path.join(outdir, 'rank%d.npz' % rank), **out)
    with limit(120, 'shutdown'):
        dist.barrier()
        dist.destroy_process_group()
