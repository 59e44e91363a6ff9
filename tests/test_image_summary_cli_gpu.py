"""train.py with `[summary] image` and `image_max`: the run's event file holds one PNG per matched stored activation with the expected tag,
height, width and colorspace; without the keys it holds no image value."""
import glob
import os
import subprocess
import sys
import tempfile

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the reference's commented image pattern
PATTERN = r'[_\w\d]+\/(input|conv\d*\/(convolution|leaky_relu\/data))$'


def _train(tmp_path, overlays):
    cmd = [sys.executable, 'train.py', '-c', 'config.ini', 'config/yolo2/tiny-20.ini'] + overlays + \
          ['--data', 'synthetic', '-b', '2', '-s', '2', '-d', '--seed', '1', '-n', 'run0']
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, 'FAILED: %s\n--- stdout\n%s\n--- stderr\n%s' % (' '.join(cmd), r.stdout[-3000:], r.stderr[-3000:])
    (path,) = glob.glob(os.path.join(str(tmp_path), 'yolo2', 'tiny', '20', 'run0', 'events.out.tfevents.*'))
    from yolo_tf_amd.utils import events
    return events.read_events(path), r.stderr


def test_event_file_with_and_without_the_image_keys(tmp_path):
    sys.path.insert(0, ROOT)
    from bench import make_builder
    from yolo_tf_amd.summary import ImageSummaries
    from yolo_tf_amd.utils import events, png
    from test_image_summary_cpu import _FakeSession, _config
    base = tmp_path / 'local.ini'
    base.write_text('[config]\nbasedir = %s\n' % tmp_path)
    keys = tmp_path / 'summary.ini'
    keys.write_text('[summary]\nimage = %s\nimage_max = 1\n' % PATTERN)
    graph = make_builder('tiny', 20, 416, True, tempfile.mkdtemp(prefix='image_summary_cli_'))[0].graph
    matched = dict((n, t) for n, t in ImageSummaries(_FakeSession(graph), _config(PATTERN, 1)).resolve())
    assert 'yolo2_tiny/input' in matched and len(matched) == 17

    evs, _ = _train(tmp_path, [str(base), str(keys)])
    with_images = [ev for ev in evs if ev['images']]
    assert with_images and with_images[-1]['step'] == 2
    last = with_images[-1]
    assert not last['scalars'] and not last['histograms']
    scalar_events = [ev for ev in evs if [t for t, _ in ev['scalars']] == list(events.SCALAR_TAGS)]
    assert scalar_events and scalar_events[-1]['step'] == 2 and not scalar_events[-1]['images']
    got = dict(last['images'])
    assert len(got) == len(last['images']) and got
    # every image belongs to a matched tensor; the ones the forward never stores (fused with their max pool) are absent
    assert set(got) <= set(n + '/image' for n in matched) and 'yolo2_tiny/input/image' in got and len(got) >= 8
    blank = 0
    for tag, im in got.items():
        t = matched[tag[:-len('/image')]]
        depth = 3 if t.c == 3 else 1
        assert (im['height'], im['width'], im['colorspace']) == (t.h, t.w, depth), tag
        pix = png.decode(im['encoded_image_string'])
        assert pix.shape == (t.h, t.w, depth), tag
        blank += pix.min() == pix.max()
    assert blank < len(got) // 2

    evs, err = _train(tmp_path, [str(base)])          # the same command without the overlay: no image value
    assert all(not ev['images'] for ev in evs) and any(ev['scalars'] for ev in evs)
    assert 'summary_image disabled' in err
