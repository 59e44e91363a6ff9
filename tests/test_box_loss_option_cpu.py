"""The `box_loss` option without a GPU: the config key and the constructor argument, the refusal of unknown values and of the YOLO (v1) family
before any device work, the C entries' argument check, and the documents that must name the option."""
import configparser
import os
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config(value=None):
    c = configparser.ConfigParser()
    c.add_section('mi355x')
    if value is not None:
        c.set('mi355x', 'box_loss', value)
    return c


def test_option_parsing():
    from yolo_tf_amd.session import BOX_LOSSES, box_loss_option
    from yolo_tf_amd import _lib
    assert BOX_LOSSES == ('mse', 'iou', 'giou', 'diou', 'ciou') and [_lib.BOX_LOSSES[k] for k in BOX_LOSSES] == [0, 1, 2, 3, 4]
    assert box_loss_option(None, None) == 'mse' and box_loss_option(None, _config()) == 'mse'
    assert box_loss_option(None, _config('CIoU')) == 'ciou' and box_loss_option('giou', _config('ciou')) == 'giou'
    for bad in ('l1', '', 'smooth'):
        with pytest.raises(ValueError, match='box_loss'):
            box_loss_option(bad, None)
    with pytest.raises(ValueError, match='box_loss'):
        box_loss_option(None, _config('eiou'))


def test_shipped_config_leaves_the_key_commented_out():
    c = configparser.ConfigParser()
    c.read(os.path.join(ROOT, 'config.ini'))
    assert not c.has_option('mi355x', 'box_loss')
    assert '; box_loss = ciou' in open(os.path.join(ROOT, 'config.ini')).read()


def test_yolo_v1_is_refused_before_device_work():
    from yolo_tf_amd import utils
    from yolo_tf_amd.model import yolo
    from yolo_tf_amd.session import TrainSession
    with tempfile.TemporaryDirectory() as d:
        cfg = utils.make_config([os.path.join(ROOT, 'config.ini'), os.path.join(ROOT, 'config', 'yolo', 'tiny-20.ini')], d)
        cfg.set('cache', 'names', os.path.join(ROOT, cfg.get('cache', 'names')))
        utils.ensure_names(cfg)
        b = yolo.Builder(None, cfg)
        b(None, training=True)
        b.create_objectives()
        with pytest.raises(NotImplementedError, match='box_loss = giou covers the YOLOv2 family'):       # (this machine has no device: nothing was touched)
            TrainSession(b, 2, dtype='f32', box_loss='giou')
        cfg.set('mi355x', 'box_loss', 'diou')
        with pytest.raises(NotImplementedError, match='box_loss = diou'):
            TrainSession(b, 2, dtype='f32', config=cfg)


def test_unknown_mode_is_an_argument_error_without_touching_the_gpu():
    import ctypes
    from yolo_tf_amd import _lib
    one = ctypes.c_void_p(64)           # never dereferenced: the check comes first
    hp = (ctypes.c_float * 4)(1, 1, 1, 1)
    for bad in (-1, 5, 99):
        with pytest.raises(_lib.HipKernelError, match='argument check failed'):
            _lib.call('yolo2_loss_box', one, 136, one, one, one, one, one, one, one, hp, one, one, one, 2, 13, 13, 5, 20, 0, None, bad)
        with pytest.raises(_lib.HipKernelError, match='argument check failed'):
            _lib.call('yolo2_loss_box_partials', one, 136, one, one, one, one, one, one, one, hp, one, one, 2, 13, 13, 5, 20, 0, None, bad)


def _args(box_loss):
    import argparse
    return argparse.Namespace(box_loss=box_loss)


def test_command_line_wins_over_the_config_key_in_both_directions():
    """train.py resolves the flag and the key once (box_loss_setting) and hands the result to the session as an argument, which wins there too."""
    import train
    from yolo_tf_amd.session import box_loss_option
    for key, flag, want in (('ciou', 'mse', 'mse'), ('mse', 'ciou', 'ciou'), ('giou', 'diou', 'diou'), ('giou', None, 'giou'), (None, None, 'mse'), (None, 'iou', 'iou')):
        cfg = _config(key)
        cfg.add_section('config')
        cfg.set('config', 'model', 'yolo2')
        got = train.box_loss_setting(_args(flag), cfg)
        assert got == want, (key, flag, got)
        assert box_loss_option(got, cfg) == want            # what TrainSession(box_loss=got, config=cfg) resolves
    cfg = _config('ciou')
    cfg.add_section('config')
    cfg.set('config', 'model', 'yolo')
    assert train.box_loss_setting(_args('mse'), cfg) == 'mse'           # YOLO (v1): --box_loss mse overrides a key that would be refused
    with pytest.raises(ValueError, match='YOLO \\(v1\\)'):
        train.box_loss_setting(_args(None), cfg)
