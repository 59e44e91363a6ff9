"""Inputs, float64 references and error bounds for the fully connected shapes of the YOLO (v1) family: `flatten` re-reads the last activation as one
pixel, so each fc layer is a 1x1 convolution with H = W = 1 and M = B rows -- 1 to 8 real rows inside a 128-row tile, several thousand input channels
behind them.  NumPy and oracle/yolo2_ref.py only: tests/test_fc_cases_cpu.py checks the cases themselves (and pins the launch rule's answer for each)
on a machine without a GPU, tests/test_fc_gpu.py launches the kernels on them.

The reference is the oracle in float64 on exactly the values a kernel reads: activations and weights rounded to bf16 first in bf16 mode
(head_cases.inputs64), the f32 bias widened unchanged, leaky-ReLU applied in float64.  Every case and every reference is built once and cached;
callers must not write to them.

Bounds are the project's own (head_cases.f32_ratio / bf16_ratio; the filter gradient's exact-product bound of tests/test_kernels_gpu.py, restated
here because that module needs a device and compared with it by tests/test_fc_gpu.py).  None is measured."""
import functools

import numpy as np

from head_cases import pad8, inputs64, f32_ratio, bf16_ratio, grad_ratio, stored, bf16_truncate, MODES, F32_RTOL      # noqa: F401  (the bounds are head_cases')
from oracle import yolo2_ref as R

ALPHA = 0.1
EPILOGUES = ('plain', 'bias', 'bias_leaky')
WS_FLOATS = 1024 + 256 * 256 * 128        # the workspace every session allocates (32 MiB + the flag words): tests/golden/conv_plans.json ws_floats
CUS = 256                                 # the CU count the launch rule is pinned at

# ------------------------------------------------------------------------------------------------------------------
# Branches of the launch rule (csrc/conv_route.hip y2_conv_route, family igemm) these shapes reach, as the plan words that tell them apart.
#   sliced    128 x 128 tile, 4 waves, 64-byte K rows, the K loop cut into grid_y > 1 slices that meet in an f32 [M][Nf] image of the workspace
#             (memset, f32 atomics, splitk_finish_kernel applies bias and leaky-ReLU)
#   wide8     128 x 128 tile, 8 waves, 128-byte K rows, one workgroup per tile
#   tail8     128 x 128 tile, 8 waves, 64-byte K rows (the channel count is no multiple of a 128-byte row; bf16: a channel tail inside a K step)
#   narrow64  Nf <= 64: 128 x 64 tile, 4 waves, one workgroup walks all of K
# ------------------------------------------------------------------------------------------------------------------
BRANCHES = {
    'sliced':   dict(BM=128, BN=128, waves=4, chunks=4, split=1),
    'wide8':    dict(BM=128, BN=128, waves=8, chunks=8, split=0),
    'tail8':    dict(BM=128, BN=128, waves=8, chunks=4, split=0),
    'narrow64': dict(BM=128, BN=64, waves=4, chunks=4, split=0),
}


def branch_of(plan):
    """Name of the branch a plan (ops.conv_route(...)['plan'] or ops.last_conv_plan()) belongs to, or None."""
    for name, words in BRANCHES.items():
        if all(plan[k] == v for k, v in words.items()) and ((plan['grid_y'] > 1) == (name == 'sliced')):
            return name
    return None


# name -> (B, Cp, real channels, Nf, kind, seed, branch with the workspace {mode: name}).  kind 'dgrad': the filter goes through filter_prep's
# transposed output, as a data gradient's does (Cp is then dY's pixel stride: 270 real channels and two zero padding lanes in the fc layer's own).
# Without a workspace, and in deterministic mode, a 'sliced' shape takes 'wide8'; the others keep their branch.
FWD_SPECS = {
    'fc_b1':        (1, 4096, 4096, 270, 'fwd', 41, {'bf16': 'sliced', 'f32': 'sliced'}),        # fc forward at B = 1: grid 3 x 16 / 3 x 32, ragged last filter tile
    'fc0_b3':       (3, 9216, 9216, 256, 'fwd', 42, {'bf16': 'sliced', 'f32': 'sliced'}),        # fc0 forward: 36 / 72 K slices
    'fc1_b8':       (8, 256, 256, 4096, 'fwd', 43, {'bf16': 'wide8', 'f32': 'wide8'}),           # fc1 forward: 32 filter tiles, unsliced
    'fc_dgrad_b2':  (2, 272, 270, 4096, 'dgrad', 44, {'bf16': 'tail8', 'f32': 'tail8'}),         # fc data gradient: channel tail
    'fc1_dgrad_b2': (2, 4096, 4096, 256, 'dgrad', 45, {'bf16': 'sliced', 'f32': 'sliced'}),      # fc1 data gradient
    'k2048_b5':     (5, 2048, 2048, 200, 'fwd', 46, {'bf16': 'wide8', 'f32': 'sliced'}),         # 64 bf16 K steps: unsliced; 128 f32 K steps: sliced
    'n40_b1':       (1, 4096, 4096, 40, 'fwd', 47, {'bf16': 'narrow64', 'f32': 'narrow64'}),     # Nf <= 64
    'n72_b1':       (1, 4096, 4096, 72, 'fwd', 48, {'bf16': 'sliced', 'f32': 'sliced'}),         # one tile, 56 of its 128 filters and 127 of its 128 rows missing
}
# (B, Cin, Cout), seed: every one the per-tap kernel (family 3) in a single pixel range (slots 1: plain stores, dW may be dirty)
WGRAD_SPECS = {
    'w_b1':       (1, 4096, 270, 51),
    'w_b1_c520':  (1, 520, 270, 52),        # 64 x 64 tiles, the last channel tile 8 wide
    'w_b3':       (3, 9216, 256, 53),
    'w_b2':       (2, 256, 4096, 54),
    'w_b8':       (8, 4096, 136, 55),
    'w_b2_big':   (2, 4096, 2048, 56),      # 512 blocks: 2 * blocks > 3 * CUs, the bf16 launch keeps the 32-pixel reduction tile; the smaller ones take the 64-pixel one
}
# (M, C, ld), seed.  ld / vec > 256 takes the one-thread-per-column kernel, else a workgroup per 16-byte channel group: both in each dtype but the first
BIAS_GRAD_SPECS = {
    'db_b1': (1, 270, 272, 61),
    'db_b3': (3, 4096, 4096, 62),
    'db_b8': (8, 1470, 1472, 63),
}
WGRAD_REL, WGRAD_FLOOR = 2e-5, 4e-6       # tests/test_kernels_gpu.py assert_wgrad_exact_products


def expected_branch(name, mode, ws=True, deterministic=False):
    b = FWD_SPECS[name][6][mode]
    return 'wide8' if b == 'sliced' and (not ws or deterministic) else b


def sliced(name, mode):
    return FWD_SPECS[name][6][mode] == 'sliced'


def k_step(mode):
    """Channels of one K step of the sliced kernel (four 16-byte chunks)."""
    return 32 if mode == 'bf16' else 16


def slice_bounds(Cp, mode, slices):
    """Channel ranges of the K slices as conv_igemm_kernel cuts them (1x1: the K order is the channel order): ceil(nk / slices) K steps each."""
    bk = k_step(mode)
    nk = -(-Cp // bk)
    per = -(-nk // slices)
    out = [(s * per * bk, min(Cp, (s + 1) * per * bk)) for s in range(slices)]
    assert all(a < b for a, b in out), (Cp, mode, slices)
    return out


# ------------------------------------------------------------------------------------------------------------------
# forward / data gradient
# ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fwd_case(name):
    """dict: B, Cp, C (real channels), Nf, ldo, kind, x f32 [B, C], w f32 [C, Nf] (the product's matrix, whichever way the filter is stored),
    bias f32 [Nf], extra f32 [C] (a row that is not part of the input: the 'one row too many' mutation)."""
    B, Cp, C, Nf, kind, seed, _ = FWD_SPECS[name]
    rng = np.random.RandomState(seed)
    x = rng.randn(B, C).astype(np.float32)
    w = (rng.randn(C, Nf) / np.sqrt(Cp)).astype(np.float32)
    bias = rng.randn(Nf).astype(np.float32)
    extra = rng.randn(C).astype(np.float32)
    for a in (x, w, bias, extra):
        a.setflags(write=False)
    return dict(name=name, B=B, Cp=Cp, C=C, Nf=Nf, ldo=pad8(Nf), kind=kind, x=x, w=w, bias=bias, extra=extra)


def _product(c, x, w, dtype):
    """The oracle's convolution of x [B, C] (as B pixels of 1 x 1) with the matrix w [C, Nf], in `dtype`."""
    t = np.dtype(dtype).type
    x4 = x.astype(t).reshape(c['B'], 1, 1, c['C'])
    if c['kind'] == 'dgrad':      # dx = dy W^T with W in HWIO = [1, 1, Nf, C]
        return R.conv2d_dgrad(x4, np.ascontiguousarray(w.astype(t).T).reshape(1, 1, c['Nf'], c['C'])).reshape(c['B'], c['Nf'])
    return R.conv2d(x4, w.astype(t).reshape(1, 1, c['C'], c['Nf'])).reshape(c['B'], c['Nf'])


def epilogue64(z, bias, epilogue):
    """bias and leaky-ReLU as the reference applies them (in z's dtype): -> (pre-activation, output)."""
    if epilogue == 'plain':
        return z, z
    pre = z + bias.astype(z.dtype)
    return pre, (R.leaky_relu(pre, ALPHA) if epilogue == 'bias_leaky' else pre)


@functools.lru_cache(maxsize=None)
def fwd_reference(name, mode, epilogue, dtype=np.float64):
    """dict: pre [B, Nf] (what leaky-ReLU sees), y [B, Nf]: the oracle in `dtype` on what the kernel reads."""
    c = fwd_case(name)
    z = _product(c, inputs64(c['x'], mode), inputs64(c['w'], mode), dtype)
    pre, y = epilogue64(z, c['bias'], epilogue)
    pre.setflags(write=False), y.setflags(write=False)
    return dict(pre=pre, y=y)


def fwd_by_slices(name, mode, epilogue, slices, drop=None, bias_each=False, leaky_each=False, extra_row=False):
    """The same result computed the way the sliced kernel does -- `slices` partial products over the channel ranges of slice_bounds, summed, then
    bias and leaky-ReLU once -- in float64, with switches for the mistakes such a kernel could make.  With every switch off it is fwd_reference.
      drop        this slice never reaches the sum
      bias_each   the bias is added once per slice
      leaky_each  leaky-ReLU is applied to each slice's partial sum (the bias riding on the first), before they meet
      extra_row   one row too many is read: `extra` is added into the last real row's input"""
    c = fwd_case(name)
    x, w = inputs64(c['x'], mode), inputs64(c['w'], mode)
    if extra_row:
        x = x.copy()
        x[-1] += inputs64(c['extra'], mode)
    bias = c['bias'].astype(np.float64) if epilogue != 'plain' else np.zeros(c['Nf'])
    leaky = (lambda v: R.leaky_relu(v, ALPHA)) if epilogue == 'bias_leaky' else (lambda v: v)
    total = np.zeros((c['B'], c['Nf']))
    for s, (a, b) in enumerate(slice_bounds(c['C'], mode, slices)):
        if s == drop:
            continue
        part = x[:, a:b] @ w[a:b]
        if bias_each or (leaky_each and s == 0):
            part = part + bias
        total += leaky(part) if leaky_each else part
    if leaky_each:
        return total
    return leaky(total if bias_each else total + bias)


def out_ratio(got, ref, mode):
    """Worst |err| / bound of a stored forward / data-gradient output: head_cases.f32_ratio, or bf16_ratio for a bf16 store."""
    return grad_ratio(got, ref, mode)


# ------------------------------------------------------------------------------------------------------------------
# filter gradient
# ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def wgrad_case(name):
    """dict: B, Cin, Cout, x f32 [B, Cin], dy f32 [B, Cout].  dy is scaled so that the largest of the B * Cin * Cout products' sums stays below 10."""
    B, Cin, Cout, seed = WGRAD_SPECS[name]
    rng = np.random.RandomState(seed)
    x = rng.randn(B, Cin).astype(np.float32)
    dy = (rng.randn(B, Cout) * (0.4 / np.sqrt(B))).astype(np.float32)
    x.setflags(write=False), dy.setflags(write=False)
    return dict(name=name, B=B, Cin=Cin, Cout=Cout, x=x, dy=dy)


def wgrad_of(c, mode, dtype=np.float64, pixels=None):
    """The oracle's filter gradient [Cin, Cout] over the listed pixels (default: all of them, once each)."""
    t = np.dtype(dtype).type
    idx = np.arange(c['B']) if pixels is None else np.asarray(pixels, np.int64)
    x, dy = inputs64(c['x'], mode)[idx].astype(t), inputs64(c['dy'], mode)[idx].astype(t)
    if len(idx) == 0:
        return np.zeros((c['Cin'], c['Cout']), t)
    return R.conv2d_wgrad(x.reshape(len(idx), 1, 1, -1), dy.reshape(len(idx), 1, 1, -1), 1, 1)[0, 0]


@functools.lru_cache(maxsize=None)
def wgrad_reference(name, mode, dtype=np.float64):
    ref = wgrad_of(wgrad_case(name), mode, dtype)
    ref.setflags(write=False)
    return ref


def wgrad_ratio(got, ref, mode):
    """Worst |err| / bound of a filter gradient: bf16 operands -- exact products, f32 accumulation -- 2e-5 |ref| + 4e-6 max|ref|
    (assert_wgrad_exact_products); f32 operands the f32 bound."""
    if mode != 'bf16':
        return f32_ratio(got, ref)
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max() + 1e-30
    return float((np.abs(got - ref) / (WGRAD_REL * np.abs(ref) + WGRAD_FLOOR * scale)).max())


# ------------------------------------------------------------------------------------------------------------------
# bias gradient
# ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bias_grad_case(name):
    """dict: M, C, ld, dy f32 [M, C] (randn / sqrt(M): unit-variance column sums)."""
    M, C, ld, seed = BIAS_GRAD_SPECS[name]
    dy = (np.random.RandomState(seed).randn(M, C) / np.sqrt(M)).astype(np.float32)
    dy.setflags(write=False)
    return dict(name=name, M=M, C=C, ld=ld, dy=dy)


@functools.lru_cache(maxsize=None)
def bias_grad_reference(name, mode, dtype=np.float64):
    ref = inputs64(bias_grad_case(name)['dy'], mode).astype(dtype).sum(0)
    ref.setflags(write=False)
    return ref
