"""Workspace form of the split filter gradients (yolo2_conv2d_wgrad_ws) on the GPU, through the C ABI: every accumulating launch shape of Darknet-19
YOLOv2 @416 at the two benchmarked batch shapes (bf16) and a handful of small f32 / odd shapes.

Per shape, with dW AND the workspace pre-filled with NaN: the result is finite and within the exact-product bound of
tests/test_bench_shapes_gpu.py::test_wgrad_bench_shape against the f64 sum of the same (bf16-exact) products,
    |got - ref| <= 2e-5 |ref| + 4e-6 max|ref|   per element
(the f32 cases take bf16-representable operands too, so their products are exact as well and the same bound holds for them)
-- the NaN fill is the teeth: an element added instead of stored, or a slot element the reducer reads but nobody wrote, comes out NaN.  Then three
calls -- the same buffers; fresh dW / ws at other addresses; a workspace 4 KiB larger, offset by 256 bytes -- must be bitwise equal: the sum's order
is a function of the plan, never of arrival or addresses."""
import numpy as np
import pytest
import torch

from oracle import yolo2_ref as R

from test_bench_shapes_gpu import CONFIGS, LAYERS, WS_FLOATS, _inputs, check_act, dev_bf16, host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from yolo_tf_amd import ops as _ops
    _ops._lib.load()
    assert torch.cuda.is_available()
    return _ops


def _bench_cases(split):
    for cname, B, head in CONFIGS:
        for name, H, cin, cout, k, bn in LAYERS:
            single = name in ('conv13_15_17', 'conv18_19', 'conv20')
            if single != split:
                marks = [pytest.mark.timeout_s(900)] if name == 'conv0' else []        # (the f64 oracle over 2.8 M pixels)
                yield pytest.param(B, name, H, H, cin, cout if cout else head, k, torch.bfloat16, id='%s-%s' % (cname, name), marks=marks)


# ragged channel and filter tiles, Cout = 125 / 425, H != W, a paired-tap shape, two shapes whose XCD-local grid has phantom blocks beyond the
# last pixel range (15 ranges in a grid of 16 per tile: tests/test_wgrad_ws_cpu.py's plan query shows blocks > ranges x tiles)
SMALL = [
    pytest.param(2, 'phantom_1x1', 32, 37, 40, 72, 1, torch.float32, id='f32-phantom-1x1'),
    pytest.param(2, 'phantom_pair', 32, 37, 24, 40, 3, torch.float32, id='f32-phantom-pair'),
    pytest.param(2, 'ragged_3x3', 16, 24, 100, 36, 3, torch.float32, id='f32-ragged-3x3'),
    pytest.param(1, 'ragged_small', 40, 40, 20, 24, 3, torch.float32, id='f32-20x24-3x3'),
    pytest.param(2, 'unaligned_slot', 37, 41, 41, 71, 1, torch.float32, id='f32-41x71-1x1'),
    pytest.param(4, 'head125', 13, 13, 1024, 125, 1, torch.bfloat16, id='bf16-b4-head125'),
    pytest.param(4, 'head425', 26, 20, 512, 425, 1, torch.bfloat16, id='bf16-head425-26x20'),
    pytest.param(2, 'row_ragged', 52, 44, 72, 136, 3, torch.bfloat16, id='bf16-row-72x136'),
]


def _operands(B, H, W, cin, cout, k, dtype, seed):
    rng = np.random.RandomState(seed)
    x, dy = rng.randn(B, H, W, cin).astype(np.float32), rng.randn(B, H, W, cout).astype(np.float32)
    vec = 8 if dtype == torch.bfloat16 else 4
    ldx, ldy = (8 if cin == 3 else (cin + vec - 1) // vec * vec), (cout + vec - 1) // vec * vec
    # bf16-representable values for BOTH dtypes: every product is then exact in f32 (the f32 kernels multiply in plain f32 MFMA), so the f64 sum of the
    # same products is THE answer and the exact-product bound applies to the f32 cases unchanged
    x, dy = torch.from_numpy(x).to(torch.bfloat16).float().numpy(), torch.from_numpy(dy).to(torch.bfloat16).float().numpy()
    if dtype == torch.bfloat16:
        return x, dy, dev_bf16(x, ldx), dev_bf16(dy, ldy), ldx, ldy

    def dev(a, ld):
        out = np.zeros(a.shape[:-1] + (ld,), np.float32)
        out[..., :a.shape[-1]] = a
        return torch.from_numpy(out).cuda().contiguous()
    return x, dy, dev(x, ldx), dev(dy, ldy), ldx, ldy


def _nan(n):
    return torch.full((n,), float('nan'), dtype=torch.float32, device='cuda')


@pytest.mark.parametrize('B,name,H,W,cin,cout,k,dtype', list(_bench_cases(True)) + SMALL)
def test_wgrad_ws_split_shape(ops, B, name, H, W, cin, cout, k, dtype):
    x, dy, xd, dyd, ldx, ldy = _operands(B, H, W, cin, cout, k, dtype, 5000 + H + cin + cout + B)
    shape = (B, H, W, cin, ldx, cout, ldy, k)
    nbytes = ops.conv2d_wgrad_workspace_bytes(*shape, dtype)
    assert nbytes > 0 and nbytes % 16 == 0 and ops.conv2d_wgrad_accumulates(*shape, dtype), 'a split shape is meant here'
    n = k * k * cin * cout
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    hplan = ops.wgrad_ws_plan(*shape, dtype, cus)
    assert nbytes == hplan['slots'] * hplan['slot_floats'] * 4

    # ---- 1. NaN everywhere: every element of dW stored, every slot element the reducer reads written by this launch
    dW, ws = _nan(n), _nan(nbytes // 4)
    ops.conv2d_wgrad_ws(xd, dyd, dW, ws, *shape)
    plan = ops.last_wgrad_plan()
    torch.cuda.synchronize()
    print('\nPLAN wgrad_ws %s: %s host plan %s' % (name, plan, hplan))
    first = dW.clone()
    assert torch.isfinite(first).all(), '%d non-finite elements' % int((~torch.isfinite(first)).sum())
    ref = R.conv2d_wgrad(x.astype(np.float64), dy.astype(np.float64), k, k)
    got = host(first).reshape(k, k, cin, cout).astype(np.float64)
    scale = float(np.abs(ref).max())
    ratio = np.abs(got - ref) / (2e-5 * np.abs(ref) + 4e-6 * scale)
    print('wgrad_ws %s: worst |err| / (2e-5 |ref| + 4e-6 scale) = %.3f' % (name, ratio.max()))
    assert ratio.max() <= 1.0, '%s: %d elements beyond the bound (worst ratio %.2f)' % (name, int((ratio > 1).sum()), ratio.max())

    # ---- 2. the plan that ran: family and slots as the host plan says, no direct store into dW by the producer
    assert plan['ranges'] == hplan['slots'] and plan['blocks'] == hplan['blocks'] and plan['direct'] == 0, (plan, hplan)
    if name == 'conv0':
        assert hplan['family'] == 0 and (plan['BC'], plan['BN'], plan['pair']) == (8, 32, 9), plan                 # the image layer's kernel
    if name == 'conv1':
        assert hplan['family'] == 1 and (plan['pair'], plan['BC'], plan['BN'], plan['waves']) == (9, 32, 64, 12), plan      # conv_wgrad_c32.hip
        assert plan['blocks'] <= cus
    if name == 'conv5_7':
        assert hplan['family'] == 2 and (plan['pair'], plan['BC'], plan['BN']) == (3, 64, 64), plan               # row kernel, variant 5
    if name in ('conv9_11', 'head125', 'head425'):
        assert hplan['family'] == 3 and plan['pair'] == 0 and plan['BC'] in (64, 128), plan                         # per-tap kernel
    if name.startswith('phantom'):
        assert hplan['family'] == 3 and plan['remap'] == 1 and plan['ranges'] % 8 != 0, plan
        tiles = (5 if name == 'phantom_pair' else -(-cin // 64) * -(-cout // 64))
        assert plan['blocks'] > plan['ranges'] * tiles, plan                                                        # blocks beyond the last range exist
        assert plan['pair'] == (1 if name == 'phantom_pair' else 0), plan
    if name == 'row_ragged':
        assert hplan['family'] == 2, hplan

    # ---- 3. three calls, bitwise equal: same buffers; fresh buffers at other addresses; a larger workspace at an offset
    ops.conv2d_wgrad_ws(xd, dyd, dW, ws, *shape)
    torch.cuda.synchronize()
    assert torch.equal(dW, first), 'same buffers, second call'
    keep = [torch.empty(12345, device='cuda'), torch.empty(777, device='cuda')]                # (moves the allocator on)
    dW2, ws2 = _nan(n), _nan(nbytes // 4)
    assert dW2.data_ptr() != dW.data_ptr() and ws2.data_ptr() != ws.data_ptr()
    ops.conv2d_wgrad_ws(xd, dyd, dW2, ws2, *shape)
    torch.cuda.synchronize()
    assert torch.equal(dW2, first), 'fresh dW / ws at other addresses'
    big = _nan(nbytes // 4 + 1024 + 64)
    ws3 = big[64:]                                                                             # 256 bytes in, 4 KiB larger
    dW3 = _nan(n)
    ops.conv2d_wgrad_ws(xd, dyd, dW3, ws3, *shape)
    torch.cuda.synchronize()
    assert torch.equal(dW3, first), 'workspace 4 KiB larger, offset by 256 bytes'
    assert torch.isnan(big[:64]).all() and torch.isnan(big[64 + nbytes // 4:]).all(), 'nothing outside the queried bytes is written'
    del keep

    # ---- 4. a workspace one byte short: an error status, dW untouched, nothing launched
    dW4 = torch.full((n,), 42.0, dtype=torch.float32, device='cuda')
    with pytest.raises(ops._lib.HipKernelError, match='code 1'):
        ops._lib.call('yolo2_conv2d_wgrad_ws', xd.data_ptr(), dyd.data_ptr(), dW4.data_ptr(), ws.data_ptr(), nbytes - 1, *shape,
                      ops.dtype_code(dtype), None)
    with pytest.raises(ops._lib.HipKernelError, match='code 1'):
        ops.conv2d_wgrad_ws(xd, dyd, dW4, None, *shape)
    torch.cuda.synchronize()
    assert bool((dW4 == 42.0).all())


@pytest.mark.parametrize('B,name,H,W,cin,cout,k,dtype', list(_bench_cases(False)) + [
    pytest.param(2, 'tiny_f32', 9, 7, 5, 7, 3, torch.float32, id='f32-5x7-3x3')])
def test_wgrad_ws_single_range_equals_the_plain_entry(ops, B, name, H, W, cin, cout, k, dtype):
    """Single-range plans store already: the query answers 0, ws may be NULL, and the result is bit for bit yolo2_conv2d_wgrad's."""
    _, _, xd, dyd, ldx, ldy = _operands(B, H, W, cin, cout, k, dtype, 6000 + cin + B)
    shape = (B, H, W, cin, ldx, cout, ldy, k)
    assert ops.conv2d_wgrad_workspace_bytes(*shape, dtype) == 0 and not ops.conv2d_wgrad_accumulates(*shape, dtype)
    n = k * k * cin * cout
    a, b = _nan(n), torch.full((n,), 3.0, dtype=torch.float32, device='cuda')
    ops.conv2d_wgrad_ws(xd, dyd, a, None, *shape)
    pa = ops.last_wgrad_plan()
    ops.conv2d_wgrad(xd, dyd, b, *shape)
    pb = ops.last_wgrad_plan()
    torch.cuda.synchronize()
    assert pa == pb and pa['direct'] == 1 and pa['ranges'] == 1, (pa, pb)
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_wgrad_ws_forced_per_tap_kernel_takes_a_row_kernel_shape(ops):
    """yolo2_debug_set_wgrad_variant(2) sends every shape to the per-tap kernel: its workspace form at a 3x3 bf16 shape the row kernel owns by rule
    (128-wide tile, eight waves), same bound, bitwise repeatable; the query follows the switch."""
    B, H, cin, cout, k = 16, 26, 256, 512, 3
    x, _, dy = _inputs(B, H, cin, cout, k, 7000)
    xd, dyd = dev_bf16(x, cin), dev_bf16(dy, cout)
    shape = (B, H, H, cin, cin, cout, cout, k)
    by_rule = ops.conv2d_wgrad_workspace_bytes(*shape, torch.bfloat16)
    ops.set_wgrad_variant(2)
    try:
        nbytes = ops.conv2d_wgrad_workspace_bytes(*shape, torch.bfloat16)
        assert nbytes > 0 and ops.conv2d_wgrad_accumulates(*shape, torch.bfloat16)
        n = k * k * cin * cout
        dW, ws = _nan(n), _nan(nbytes // 4)
        ops.conv2d_wgrad_ws(xd, dyd, dW, ws, *shape)
        plan = ops.last_wgrad_plan()
        dW2, ws2 = _nan(n), _nan(nbytes // 4)
        ops.conv2d_wgrad_ws(xd, dyd, dW2, ws2, *shape)
        torch.cuda.synchronize()
        assert (plan['BC'], plan['BN'], plan['waves'], plan['pair'], plan['direct']) == (128, 128, 8, 0, 0) and plan['ranges'] * n * 4 == nbytes, plan
    finally:
        ops.set_wgrad_variant(0)
    assert ops.conv2d_wgrad_workspace_bytes(*shape, torch.bfloat16) == by_rule
    assert torch.equal(dW, dW2)
    ref = R.conv2d_wgrad(x.astype(np.float64), dy.astype(np.float64), k, k)
    got = host(dW).reshape(k, k, cin, cout).astype(np.float64)
    assert (np.abs(got - ref) <= 2e-5 * np.abs(ref) + 4e-6 * float(np.abs(ref).max())).all()


def test_wgrad_ws_beside_a_streamk_forward_is_bitwise_the_quiet_run(ops):
    """In the manner of test_streamk_under_concurrent_row_wgrad: the split row-kernel filter gradient of a 26x26 layer on a side stream while a stream-K
    forward (13x13, 512 -> 1024: workgroups handing partial tiles through flags) runs on the main stream and takes CUs.  The filter gradient is bit for bit
    the one computed on a quiet device, the forward still correct, no give-up reported."""
    B, H, cin, cout, k = 16, 26, 256, 512, 3
    x, _, dy = _inputs(B, H, cin, cout, k, 8000)
    xd, dyd = dev_bf16(x, cin), dev_bf16(dy, cout)
    shape = (B, H, H, cin, cin, cout, cout, k)
    nbytes = ops.conv2d_wgrad_workspace_bytes(*shape, torch.bfloat16)
    n = k * k * cin * cout
    quiet, ws = _nan(n), _nan(nbytes // 4)
    ops.conv2d_wgrad_ws(xd, dyd, quiet, ws, *shape)
    assert ops.last_wgrad_plan()['pair'] == 3 and ops.last_wgrad_plan()['ranges'] > 1
    torch.cuda.synchronize()
    # the stream-K launch
    fB, fH, fcin, fcout = 16, 13, 512, 1024
    fx, fw, _ = _inputs(fB, fH, fcin, fcout, 3, 8001)
    fxd = dev_bf16(fx, fcin)
    Ff = torch.zeros(fcout * 9 * fcin, dtype=torch.bfloat16, device='cuda')
    ops.filter_prep(torch.from_numpy(fw).cuda(), Ff, None, 3, fcin, fcin, fcout, fcout, torch.bfloat16)
    cws = torch.zeros(WS_FLOATS, dtype=torch.float32, device='cuda')
    ref_y = R.conv2d(fx, fw)
    side = torch.cuda.Stream()
    busy, ws_b = _nan(n), _nan(nbytes // 4)
    O = torch.zeros(fB * fH * fH * fcout, dtype=torch.bfloat16, device='cuda')
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ops.conv2d_wgrad_ws(xd, dyd, busy, ws_b, *shape)
    ops.conv2d_ws(fxd, Ff, None, O, cws, fB, fH, fH, fcin, fcin, fcout, fcout, 3)
    plan_f = ops.last_conv_plan()
    assert plan_f['split'] == 2 and plan_f['grid_x'] > 88, plan_f            # stream-K: more workgroups than tiles
    side.synchronize()
    ops.check_async_errors()
    assert torch.equal(busy, quiet)
    check_act(host(O).reshape(fB, fH, fH, fcout), ref_y, 'stream-K forward beside the workspace-form filter gradient')
