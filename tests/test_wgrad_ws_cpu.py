"""Workspace form of the split filter gradients (yolo2_conv2d_wgrad_ws, the deterministic training mode), host side only: the workspace
query agrees with the launch plan and with yolo2_conv2d_wgrad_accumulates for every benchmarked shape, bad arguments are refused without a
launch, and the YOLO (v1) family is refused by the session and the engine before anything touches a device.

Without a GPU the library plans for 256 compute units (csrc/conv_wgrad.hip wgrad_cus), the MI355X's count; with one, for that device's.  The plan
queries below are asked for the same number."""
import os
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256

# name, H (= W), Cin, Cout, ksize -- the distinct launch shapes of Darknet-19 YOLOv2 @416 (tests/test_bench_shapes_gpu.py LAYERS); None = the head
LAYERS = [
    ('conv0', 416, 3, 32, 3), ('conv1', 208, 32, 64, 3), ('conv2_4', 104, 64, 128, 3), ('conv3', 104, 128, 64, 1), ('conv5_7', 52, 128, 256, 3),
    ('conv6', 52, 256, 128, 1), ('conv8_10_12', 26, 256, 512, 3), ('conv9_11', 26, 512, 256, 1), ('conv13_15_17', 13, 512, 1024, 3),
    ('conv14_16', 13, 1024, 512, 1), ('conv18_19', 13, 1024, 1024, 3), ('conv20', 13, 3072, 1024, 3), ('conv_out', 13, 1024, None, 1),
]
CONFIGS = [('b16_voc20', 16, 125, BF16), ('b8_coco80', 8, 425, BF16), ('b4_voc20', 4, 125, BF16), ('b16_voc20_f32', 16, 125, F32), ('b4_coco80_f32', 4, 425, F32)]
FAMILY = {'image': 0, 'conv1': 1, 'row': 2, 'per_tap': 3}


@pytest.fixture(scope='module')
def ops():
    from yolo_tf_amd import ops as _ops
    _ops._lib.load()
    return _ops


def pad(c, dtype):
    v = 8 if dtype == BF16 else 4
    return (c + v - 1) // v * v


def _cases():
    for cname, B, head, dtype in CONFIGS:
        for name, H, cin, cout, k in LAYERS:
            yield pytest.param(B, dtype, name, H, cin, cout if cout else head, k, id='%s-%s' % (cname, name))


@pytest.mark.parametrize('B,dtype,name,H,cin,cout,k', list(_cases()))
def test_workspace_bytes_match_the_plan_and_the_accumulates_query(ops, B, dtype, name, H, cin, cout, k):
    q = ops._lib.query
    tdtype = torch.bfloat16 if dtype == BF16 else torch.float32
    ldx, ldy = (8 if cin == 3 else pad(cin, dtype)), pad(cout, dtype)          # (the image is stored 8 channels wide)
    nbytes = ops.conv2d_wgrad_workspace_bytes(B, H, H, cin, ldx, cout, ldy, k, tdtype)
    accumulates = q('yolo2_conv2d_wgrad_accumulates', B, H, H, cin, ldx, cout, ldy, k, dtype)
    assert (nbytes > 0) == (accumulates == 1), (nbytes, accumulates)
    plan = ops.wgrad_ws_plan(B, H, H, cin, ldx, cout, ldy, k, tdtype, CUS)
    slot_floats = (k * k * cin * cout + 3) // 4 * 4                            # one filter gradient, rounded up to 16 bytes
    assert plan['slot_floats'] == slot_floats
    assert nbytes == (plan['slots'] * slot_floats * 4 if plan['slots'] > 1 else 0)
    assert plan['slots'] >= 1 and plan['blocks'] >= plan['slots']
    # the slots are what the launch's own host plan reports: pixel ranges of the row kernel, workgroups of conv1's kernel and the image layer's
    if plan['family'] == FAMILY['row']:
        import ctypes
        out = (ctypes.c_int * 9)()
        assert q('yolo2_debug_wgrad_row_plan', B, H, H, cin, cout, CUS, -1, out) == 0
        assert out[0] >= 0 and out[1] == plan['slots'] and out[3] == plan['blocks'] and bool(out[5]) == (plan['slots'] == 1)
    if plan['family'] in (FAMILY['conv1'], FAMILY['image']):
        assert plan['blocks'] == plan['slots']
    # which family takes which layer (bf16: the product path; f32: the image layer's kernel and the per-tap kernel only)
    if name == 'conv0':
        assert plan['family'] == FAMILY['image'] and 8 <= plan['slots'] <= 512 and plan['slots'] % 8 == 0
    elif dtype == F32 or k == 1:
        assert plan['family'] == FAMILY['per_tap']
    elif name == 'conv1':
        assert plan['family'] == FAMILY['conv1'] and 1 < plan['slots'] <= CUS
    else:
        assert plan['family'] == FAMILY['row']
    if dtype == BF16 and B in (8, 16):
        # what the issue counts: the three 13x13 3x3 shapes take one range and store, the other ten shapes split
        assert (plan['slots'] == 1) == (name in ('conv13_15_17', 'conv18_19', 'conv20')), (name, plan)


def test_small_and_odd_shapes(ops):
    # ragged channel and filter tiles, H != W, unaligned filter sizes: the slot stride is rounded up to 16 bytes
    for B, H, W, cin, cout, k, dtype in [(2, 7, 9, 5, 7, 3, torch.float32), (3, 10, 6, 20, 12, 1, torch.float32), (2, 12, 20, 72, 136, 3, torch.bfloat16),
                                         (1, 5, 5, 3, 5, 1, torch.float32), (4, 26, 26, 512, 425, 1, torch.bfloat16)]:
        code = BF16 if dtype == torch.bfloat16 else F32
        ldx, ldy = pad(cin, code), pad(cout, code)
        plan = ops.wgrad_ws_plan(B, H, W, cin, ldx, cout, ldy, k, dtype, CUS)
        nbytes = ops.conv2d_wgrad_workspace_bytes(B, H, W, cin, ldx, cout, ldy, k, dtype)
        assert plan['slot_floats'] % 4 == 0 and 0 <= plan['slot_floats'] - k * k * cin * cout < 4
        assert nbytes == (plan['slots'] * plan['slot_floats'] * 4 if plan['slots'] > 1 else 0)
        assert (nbytes > 0) == bool(ops.conv2d_wgrad_accumulates(B, H, W, cin, ldx, cout, ldy, k, dtype))


def test_bad_arguments_are_refused_without_a_launch(ops):
    import ctypes
    q, lib = ops._lib.query, ops._lib.load()
    good = (16, 26, 26, 256, 256, 512, 512, 3, BF16)
    assert q('yolo2_conv2d_wgrad_workspace_bytes', *good) > 0
    for i, bad in [(0, 0), (1, -1), (3, 0), (4, 8), (4, 260), (6, 500), (7, 2), (7, 5), (8, 7)]:      # batch, H, Cin, ldx < Cin, ldx % 8, ldy < Cout, ksize, dtype
        args = list(good)
        args[i] = bad
        assert q('yolo2_conv2d_wgrad_workspace_bytes', *args) == 0, args
        out = (ctypes.c_int * 4)()
        assert lib.yolo2_debug_wgrad_ws_plan(*(args + [CUS, out])) == 1, args                          # YOLO2_E_ARG
    out = (ctypes.c_int * 4)()
    assert lib.yolo2_debug_wgrad_ws_plan(*(list(good) + [0, out])) == 1 and lib.yolo2_debug_wgrad_ws_plan(*(list(good) + [CUS, None])) == 1
    # the entry itself: null operands and a missing / short workspace are argument errors (status 1), raised before any launch
    with pytest.raises(ops._lib.HipKernelError, match='code 1'):
        ops._lib.call('yolo2_conv2d_wgrad_ws', None, None, None, None, 0, *(list(good) + [None]))
    with pytest.raises(ops._lib.HipKernelError, match='code 1'):
        ops._lib.call('yolo2_conv2d_wgrad_ws', 4096, 4096, 4096, None, 0, *(list(good) + [None]))         # split plan, no workspace
    with pytest.raises(ops._lib.HipKernelError, match='code 1'):
        ops._lib.call('yolo2_conv2d_wgrad_ws', 4096, 4096, 4096, 4096, q('yolo2_conv2d_wgrad_workspace_bytes', *good) - 1, *(list(good) + [None]))


def test_deterministic_flag_is_per_thread_and_off_by_default(ops):
    import threading
    q = ops._lib.query
    assert q('yolo2_get_deterministic') == 0
    ops.set_deterministic(True)
    seen = []
    t = threading.Thread(target=lambda: seen.append(q('yolo2_get_deterministic')))
    t.start()
    t.join()
    assert q('yolo2_get_deterministic') == 1 and seen == [0]
    ops.set_deterministic(False)
    assert q('yolo2_get_deterministic') == 0


def test_deterministic_launches_restores_the_mode_it_found(ops):
    q = ops._lib.query
    with ops.deterministic_launches(True):
        with ops.deterministic_launches(True):
            assert q('yolo2_get_deterministic') == 1
        assert q('yolo2_get_deterministic') == 1            # the inner block left the outer one's mode alone
        with ops.deterministic_launches(False):
            assert q('yolo2_get_deterministic') == 1        # a default engine never touches the switch
    assert q('yolo2_get_deterministic') == 0
    ops.set_deterministic(True)                              # a caller that set the mode itself keeps it
    with ops.deterministic_launches(True):
        pass
    assert q('yolo2_get_deterministic') == 1
    ops.set_deterministic(False)


def test_fixed_order_clip_workspace_and_argument_checks(ops):
    assert ops.workspace_bytes('clip_fixed', 66) == 66 * 64 * 8 and ops.workspace_bytes('clip_fixed', 0) == 0
    with pytest.raises(ops._lib.HipKernelError, match='code 1'):      # a workspace one byte short: refused before any launch
        ops._lib.call('yolo2_clip_by_norm_fixed', 4096, 4096, 66, 5.0, 4096, 66 * 64 * 8 - 1, None)


def _v1_builder(basedir):
    from yolo_tf_amd import utils
    from yolo_tf_amd.model import yolo
    cfg = utils.make_config([os.path.join(ROOT, 'config.ini'), os.path.join(ROOT, 'config', 'yolo', 'tiny-20.ini')], basedir)
    cfg.set('cache', 'names', os.path.join(ROOT, cfg.get('cache', 'names')))
    utils.ensure_names(cfg)
    b = yolo.Builder(None, cfg)
    b(None, training=True)
    b.create_objectives()
    return b


def test_deterministic_mode_refuses_the_v1_family():
    from yolo_tf_amd.engine import Engine
    from yolo_tf_amd.session import TrainSession
    with tempfile.TemporaryDirectory() as d:
        b = _v1_builder(d)
        with pytest.raises(NotImplementedError, match='YOLOv2'):
            TrainSession(b, 2, dtype='f32', deterministic=True)
        with pytest.raises(NotImplementedError, match='YOLOv2'):
            Engine(b.graph, 2, 'f32', training=True, deterministic=True)
