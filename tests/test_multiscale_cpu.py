"""Multi-scale training without a GPU: the size-list parser, the schedule as a pure function of the global step, the configuration keys and
the command line's flags (yolo_tf_amd/multiscale.py, train.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config(*overlays, **mi355x):
    from yolo_tf_amd import utils
    cfg = utils.make_config([os.path.join(ROOT, 'config.ini')] + [os.path.join(ROOT, o) for o in overlays])
    for k, v in mi355x.items():
        if not cfg.has_section('mi355x'):
            cfg.add_section('mi355x')
        cfg.set('mi355x', k, str(v))
    return cfg


def test_module_imports_without_torch():
    code = 'import sys; from yolo_tf_amd import multiscale; assert "torch" not in sys.modules; print("ok")'
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stderr[-2000:]


def test_range_gives_the_ten_squares():
    from yolo_tf_amd.multiscale import parse_sizes
    assert parse_sizes('320-608', 32, 32) == [(s, s) for s in range(320, 609, 32)]
    assert parse_sizes('64-128', 32, 32) == [(64, 64), (96, 96), (128, 128)]
    assert parse_sizes('416-416', 32, 32) == [(416, 416)]


def test_mixed_entries_duplicates_order_and_empty():
    from yolo_tf_amd.multiscale import parse_sizes
    assert parse_sizes('416 320x352', 32, 32) == [(320, 352), (416, 416)]
    assert parse_sizes('416, 320x352,416  352x320 320-352', 32, 32) == [(320, 320), (320, 352), (352, 320), (352, 352), (416, 416)]     # (area, width)
    assert parse_sizes('608,320', 32, 32) == [(320, 320), (608, 608)]
    assert parse_sizes('128x64', 64, 32) == [(128, 64)] and parse_sizes('64-192', 64, 32) == [(64, 64), (128, 128), (192, 192)]
    assert parse_sizes('', 32, 32) == [] and parse_sizes('  ', 32, 32) == [] and parse_sizes(None, 32, 32) == [] and parse_sizes(' , ', 32, 32) == []


@pytest.mark.parametrize('spec,needles', [('300', ['300', '32']), ('320x300', ['320x300', '32']), ('320-600', ['320-600', '32']), ('608-320', ['608-320']),
                                          ('big', ['big']), ('320x', ['320x']), ('0', ['0', '32']), ('416 -32', ['-32'])])
def test_bad_entries_name_the_entry_and_the_stride(spec, needles):
    from yolo_tf_amd.multiscale import parse_sizes
    with pytest.raises(ValueError) as e:
        parse_sizes(spec, 32, 32)
    assert all(n in str(e.value) for n in needles), str(e.value)


def test_height_is_checked_against_its_own_stride():
    from yolo_tf_amd.multiscale import parse_sizes
    assert parse_sizes('64x48', 32, 16) == [(64, 48)]
    with pytest.raises(ValueError) as e:
        parse_sizes('64x40', 32, 16)
    assert '16' in str(e.value) and '64x40' in str(e.value)


def test_schedule_is_the_stated_pure_function():
    from yolo_tf_amd.multiscale import SizeSchedule
    sizes = [(64, 64), (96, 96), (128, 128)]
    s = SizeSchedule(sizes, 2, 0)
    assert [sizes.index(s.at(g)) for g in range(8)] == [0, 0, 1, 1, 0, 0, 2, 2]            # blocks 0-3 draw 0, 1, 0, 2
    for seed, every, g in [(0, 2, 5), (3, 10, 1234), (7, 1, 99), (2 ** 20, 3, 2 ** 31)]:
        want = sizes[np.random.RandomState((seed * 1000003 + g // every) % 2 ** 32).randint(len(sizes))]
        assert SizeSchedule(sizes, every, seed).at(g) == want


def test_schedule_is_constant_within_a_block_and_has_no_memory_and_no_rank():
    from yolo_tf_amd.multiscale import SizeSchedule
    sizes = [(s, s) for s in range(320, 609, 32)]
    a, b = SizeSchedule(sizes, 10, 5), SizeSchedule(sizes, 10, 5)        # two ranks of one run: the same arguments, nothing else to give
    forward = [a.at(g) for g in range(200)]
    assert all(len(set(forward[i:i + 10])) == 1 for i in range(0, 200, 10))
    assert len(set(forward)) > 1
    backward = [b.at(g) for g in reversed(range(200))][::-1]             # another call history, e.g. a run resumed at any step
    assert backward == forward and [a.at(g) for g in (150, 3, 150, 77)] == [forward[g] for g in (150, 3, 150, 77)]
    np.random.seed(1)                                                     # the global generator is neither read nor advanced
    state = np.random.get_state()[1].copy()
    assert a.at(42) == forward[42] and np.array_equal(np.random.get_state()[1], state)
    assert [SizeSchedule(sizes, 10, 6).at(g) for g in range(200)] != forward


def test_every_size_appears_over_2000_steps():
    from yolo_tf_amd.multiscale import SizeSchedule
    sizes = [(s, s) for s in range(320, 609, 32)]
    s = SizeSchedule(sizes, 10, 0)
    assert set(s.at(g) for g in range(2000)) == set(sizes)


def test_schedule_refuses_every_below_one_and_an_empty_list():
    from yolo_tf_amd.multiscale import SizeSchedule
    for every in (0, -3):
        with pytest.raises(ValueError) as e:
            SizeSchedule([(64, 64)], every, 0)
        assert 'multiscale_every' in str(e.value)
    with pytest.raises(ValueError):
        SizeSchedule([], 10, 0)


def test_config_without_the_key_gives_no_schedule():
    from yolo_tf_amd import multiscale
    assert multiscale.configure(_config('config/yolo2/tiny-20.ini')) is None
    assert multiscale.configure(_config('config/yolo2/tiny-20.ini', multiscale='')) is None
    assert multiscale.configure(_config('config/yolo2/tiny-20.ini', multiscale='  ', multiscale_every=3)) is None
    assert multiscale.configure(_config('config/yolo2/tiny-20.ini', multiscale='320-608'), spec='') is None      # the flag turns the key off
    assert multiscale.configure(_config('config/yolo/tiny-20.ini')) is None                                      # v1 without the key: as before


def test_config_keys_overrides_and_the_configured_size():
    from yolo_tf_amd import multiscale
    cfg = _config('config/yolo2/tiny-20.ini', multiscale='320-608')
    own = (cfg.getint('yolo2', 'width'), cfg.getint('yolo2', 'height'))
    assert own == (416, 416)
    assert multiscale.configure(cfg) == ([(s, s) for s in range(320, 609, 32)], 10, False)                      # the paper's ten steps by default
    cfg.set('mi355x', 'multiscale_every', '4')
    assert multiscale.configure(cfg)[1] == 4 and multiscale.configure(cfg, every=7)[1] == 7
    assert multiscale.configure(cfg, spec='64 128', every=2) == ([(64, 64), (128, 128), (416, 416)], 2, True)    # the configured size joins the list
    assert multiscale.describe([(64, 64), (128, 96)]) == '64 128x96'


def test_refusals_name_the_key_and_the_reason():
    from yolo_tf_amd import multiscale
    with pytest.raises(ValueError) as e:
        multiscale.configure(_config('config/yolo/tiny-20.ini', multiscale='448'))
    assert '[mi355x] multiscale' in str(e.value) and 'fully connected' in str(e.value)
    with pytest.raises(ValueError) as e:
        multiscale.configure(_config('config/yolo2/tiny-20.ini'), spec='100')
    assert '[mi355x] multiscale' in str(e.value) and "'100'" in str(e.value) and '32' in str(e.value)
    with pytest.raises(ValueError) as e:
        multiscale.configure(_config('config/yolo2/tiny-20.ini', multiscale='320-608', multiscale_every=0))
    assert 'multiscale_every' in str(e.value)
    with pytest.raises(ValueError) as e:
        multiscale.configure(_config('config/yolo2/tiny-20.ini'), spec='320x640 640x320')       # neither contains the other (nor 416x416 both)
    assert 'largest' in str(e.value)


def test_follow_binds_the_session_and_logs_only_changes():
    from yolo_tf_amd import multiscale

    class Session(object):
        size, global_step, calls = (96, 96), 0, []

        def set_size(self, w, h):
            self.calls.append((self.global_step, (w, h)))
            self.size = (w, h)

    class Log(object):
        lines = []

        def warning(self, line):
            self.lines.append(line)
    s, log = Session(), Log()
    assert multiscale.follow(s, None, log) == (96, 96) and s.calls == [] and log.lines == []
    schedule = multiscale.SizeSchedule([(64, 64), (96, 96), (128, 128)], 2, 0)
    visited = []
    for g in range(8):
        s.global_step = g
        visited.append(multiscale.follow(s, schedule, log))
    assert visited == [schedule.at(g) for g in range(8)]
    assert s.calls == [(0, (64, 64)), (2, (96, 96)), (4, (64, 64)), (6, (128, 128))]
    assert log.lines == ['step 0: input size 64x64', 'step 2: input size 96x96', 'step 4: input size 64x64', 'step 6: input size 128x128']


def test_train_make_args_accepts_the_two_flags():
    sys.path.insert(0, ROOT)
    import train
    args = train.make_args(['--multiscale', '320-608', '--multiscale_every', '5'])
    assert args.multiscale == '320-608' and args.multiscale_every == 5
    args = train.make_args([])
    assert args.multiscale is None and args.multiscale_every is None
    assert train.multiscale_setting(args, _config('config/yolo2/tiny-20.ini')) is None


def test_eval_make_args_accepts_sizes():
    sys.path.insert(0, ROOT)
    import eval as eval_cli
    assert eval_cli.make_args(['--sizes', '64 128']).sizes == '64 128' and eval_cli.make_args([]).sizes is None
