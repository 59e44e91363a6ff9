"""ImageSummaries over a real training step: the image of every stored activation of the tiny network, made on the device, equals the
specification (tests/image_summary_ref.py) applied to a host copy of the same tensor with the padding stripped."""
import os
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_summary_ref as R  # noqa: E402
from test_image_summary_cpu import _config  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _session(dtype):
    import torch
    sys.path.insert(0, ROOT)
    from bench import make_builder
    from yolo_tf_amd.session import TrainSession
    from yolo_tf_amd.utils import data
    B, size = 2, 96
    b, _ = make_builder('tiny', 20, size, True, tempfile.mkdtemp(prefix='image_summary_engine_'))
    sess = TrainSession(b, B, dtype=dtype, optimizer='adam', learning_rate=1e-3, seed=3)
    images = torch.rand(B, size, size, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(0)) * 255
    sess.step(images, data.synthetic_batch(B, 20, size // 32, size // 32, seed=1))
    return sess, B


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
def test_images_of_one_step_match_the_specification(dtype):
    from yolo_tf_amd.summary import ImageSummaries, activation_tag
    sess, B = _session(dtype)
    e = sess.engine
    inputs = set(e.graph.inputs.values())
    # host copies of the stored activations, padding stripped: [B, h, w, c] f32
    want, skipped = {}, []
    for t, where in e.summarizable_tensors():
        name = activation_tag(t.name, 'yolo2_tiny', t in inputs)
        if where is None:
            skipped.append(name)
            continue
        buf, rows, c, ld = where
        a = buf[:(rows - 1) * ld + c].float().cpu().numpy()
        a = np.concatenate([a, np.zeros(ld - c, a.dtype)]).reshape(rows, ld)[:, :c]
        want[name] = a.reshape(B, t.h, t.w, c).copy()
    assert len(want) >= 10 and len(skipped) >= 1              # the layers fused with their max pool never store their activation
    assert want['yolo2_tiny/input'].shape == (B, 96, 96, 3) and 'yolo2_tiny/conv0/convolution' in want
    first = None
    for image_max in (1, 3):
        s = ImageSummaries(sess, _config('.*', image_max))     # `.*` matches the variables and moments too: skipped with a warning
        s.collect()
        got = s.results()
        tags = [g[0] for g in got]
        assert len(set(tags)) == len(tags)
        expected = {}
        for name, x in want.items():
            for tag, pix, info in R.image_summary(name, x, image_max):
                expected[tag] = (pix, info)
        assert sorted(tags) == sorted(expected)                 # skipped tensors, variables and moments are absent
        assert not [t for t in tags if any(t.startswith(n + '/image') for n in skipped)]
        records = dict(s.records)
        for tag, h, w, depth, pix in got:
            ref, info = expected[tag]
            assert (h, w, depth) == ref.shape and pix.dtype == np.uint8, tag
            assert np.array_equal(pix, ref), (tag, np.argwhere(pix != ref)[:4])
            assert records[tag]['min'] == info['min'] and records[tag]['max'] == info['max'] and records[tag]['nonfinite'] == info['nonfinite'] == 0, tag
            assert np.float32(records[tag]['scale']) == np.float32(info['scale']), tag
        depths = dict((g[0], g[3]) for g in got)
        assert depths['yolo2_tiny/input/image' + ('' if image_max == 1 else '/0')] == 3
        assert depths['yolo2_tiny/conv0/convolution/image' + ('' if image_max == 1 else '/1')] == 1
        assert len(got) == len(want) * min(image_max, B)
        # a second collection of the unchanged state: the same bytes
        s.collect()
        again = s.results()
        assert [g[:4] for g in again] == [g[:4] for g in got] and all(np.array_equal(a[4], g[4]) for a, g in zip(again, got))
        if first is None:
            first = dict((g[0], g[4]) for g in got)
        else:                                                   # image 0 does not depend on how many images are asked for
            assert all(np.array_equal(first[n + '/image'], dict((g[0], g[4]) for g in got)[n + '/image/0']) for n in want)
    assert any(p.min() < p.max() for p in first.values())       # (not all of them blank)


def test_disabled_instance_allocates_and_launches_nothing(monkeypatch):
    import torch
    from yolo_tf_amd import _lib, ops, summary
    sess, _ = _session('bf16')
    calls = []
    monkeypatch.setattr(ops, 'call', lambda name, *a: calls.append(name) or _lib.call(name, *a))
    monkeypatch.setattr(ops, 'ImageJobs', lambda *a, **k: pytest.fail('a disabled instance built a job table'))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for cfg in (_config(), _config('.*'), _config(image_max=2), _config('.*', 1, key='image_'), None):
        s = summary.ImageSummaries(sess, cfg)
        assert not s.enabled
        s.collect()
        assert s.results() == [] and s._plans == {} and s._pending is None
    assert calls == [] and torch.cuda.memory_allocated() == before
