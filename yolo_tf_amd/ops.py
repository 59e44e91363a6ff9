"""Thin tensor-level wrappers over the C-ABI kernels (torch tensors are only device memory +
stream plumbing here).  Used by the engine and by the per-kernel parity tests."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, dtype_code


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_raw_device = getattr(torch._C, '_cuda_getDevice', None)


def _stream():
    """The current HIP stream of the current device as a raw handle.  torch.cuda.current_stream() builds a Stream object through four
    Python layers (device-index parsing, is_available(), lazy-init checks): ~8 us per call, as much as the kernel launch itself and 28 %
    of the host time of a training step (scripts/host_profile.py); the two C accessors cost ~0.3 us together."""
    if _raw_stream is None or _raw_device is None:
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return ctypes.c_void_p(_raw_stream(_raw_device()))


def pad8(c):
    return (c + 7) // 8 * 8


def conv2d(P, F, bias, O, B, H, W, Cp, ldp, Nf, ldo, ksize):
    call('yolo2_conv2d', ptr(P), ptr(F), ptr(bias), ptr(O), B, H, W, Cp, ldp, Nf, ldo, ksize, dtype_code(P.dtype), _stream())


def _ws_bytes(ws):
    return 0 if ws is None else ws.numel() * ws.element_size()


def conv2d_ws(P, F, bias, O, ws, B, H, W, Cp, ldp, Nf, ldo, ksize):
    """``ws``: f32 tensor, or None -- the launch rule then only names kernels that need no workspace (as ``conv2d``)."""
    call('yolo2_conv2d_ws', ptr(P), ptr(F), ptr(bias), ptr(O), ptr(ws), _ws_bytes(ws), B, H, W, Cp, ldp, Nf, ldo, ksize,
         dtype_code(P.dtype), _stream())


def conv2d_bias_leaky(P, F, bias, O, ws, B, H, W, Cp, ldp, Nf, ldo, ksize, alpha):
    """``ws``: as for ``conv2d_ws``."""
    call('yolo2_conv2d_bias_leaky', ptr(P), ptr(F), ptr(bias), ptr(O), ptr(ws), _ws_bytes(ws), B, H, W, Cp, ldp, Nf, ldo, ksize,
         alpha, dtype_code(P.dtype), _stream())


def conv2d_bn(P, F, O, ws, B, H, W, Cp, ldp, Nf, ldo, ksize, shift, bn_part):
    call('yolo2_conv2d_bn', ptr(P), ptr(F), ptr(O), ptr(ws), ws.numel() * ws.element_size(), B, H, W, Cp, ldp, Nf, ldo, ksize,
         ptr(shift), ptr(bn_part), dtype_code(P.dtype), _stream())


def conv2d_dgrad_bn(dY, F, dX, ws, B, H, W, Cp, ldp, Nf, ldo, ksize, Yprev, mean, var, gamma, beta, dgamma, dbeta, bn_part, red_ws, eps, alpha):
    """-> True when the sums are still in ``bn_part`` (finish with ``bn_part_to_grads``)."""
    pending = ctypes.c_int(0)
    call('yolo2_conv2d_dgrad_bn', ptr(dY), ptr(F), ptr(dX), ptr(ws), ws.numel() * ws.element_size(), B, H, W, Cp, ldp, Nf, ldo, ksize,
         ptr(Yprev), ptr(mean), ptr(var), ptr(gamma), ptr(beta), ptr(dgamma), ptr(dbeta), ptr(bn_part), ptr(red_ws), eps, alpha,
         ctypes.byref(pending), dtype_code(dY.dtype), _stream())
    return bool(pending.value)


def conv2d_dgrad_bn_fuses(B, H, W, Nf, ksize, dtype):
    """Would ``conv2d_dgrad_bn`` take the producer's sums from its epilogue for this data gradient?  (False: the launch rule prefers a plain data
    gradient there; the caller schedules ``bn_leaky_bwd_reduce_part`` + ``bn_leaky_bwd_apply_fin`` itself.)"""
    lib = _lib.load()
    if 'yolo2_conv2d_dgrad_bn_fuses' in _lib.MISSING:       # (an earlier round's library, YOLO2_LIB_BASELINE=1: it always fused)
        return True
    return bool(lib.yolo2_conv2d_dgrad_bn_fuses(B, H, W, Nf, ksize, dtype_code(dtype)))


def filter_prep_blocks(ksize, ldcin, ldcout):
    """Workgroups one layer takes in ``filter_prep_batch`` / ``adam_filter_prep`` (the layer's ``first_block`` arithmetic)."""
    lib = _lib.load()
    if 'yolo2_filter_prep_blocks' in _lib.MISSING:       # (an earlier round's library, YOLO2_LIB_BASELINE=1: 64 x 64 tiles)
        return ksize * ksize * ((ldcin + 63) // 64) * ((ldcout + 63) // 64)
    return int(lib.yolo2_filter_prep_blocks(ksize, ldcin, ldcout))


def bn_part_to_grads(bn_part, C, dgamma, dbeta):
    call('yolo2_bn_part_to_grads', ptr(bn_part), C, ptr(dgamma), ptr(dbeta), _stream())


def bn_finalize(bn_part, shift, M, C, mean, var, mm, mv, decay):
    call('yolo2_bn_finalize', ptr(bn_part), ptr(shift), M, C, ptr(mean), ptr(var), ptr(mm), ptr(mv), decay, _stream())


def conv2d_wgrad_accumulates(B, H, W, Cin, ldx, Cout, ldy, ksize, dtype):
    """True when yolo2_conv2d_wgrad adds into dW with atomics for this shape (dW must be zeroed first); False when it overwrites."""
    return bool(_lib.load().yolo2_conv2d_wgrad_accumulates(B, H, W, Cin, ldx, Cout, ldy, ksize, dtype_code(dtype)))


def conv2d_wgrad(X, dY, dW, B, H, W, Cin, ldx, Cout, ldy, ksize):
    call('yolo2_conv2d_wgrad', ptr(X), ptr(dY), ptr(dW), B, H, W, Cin, ldx, Cout, ldy, ksize, dtype_code(X.dtype), _stream())


def conv2d_wgrad_workspace_bytes(B, H, W, Cin, ldx, Cout, ldy, ksize, dtype):
    """Bytes of workspace ``conv2d_wgrad_ws`` needs for this shape (0: a single pixel range, plain stores already)."""
    return int(_lib.query('yolo2_conv2d_wgrad_workspace_bytes', B, H, W, Cin, ldx, Cout, ldy, ksize, dtype_code(dtype)))


def conv2d_wgrad_ws(X, dY, dW, ws, B, H, W, Cin, ldx, Cout, ldy, ksize):
    """Filter gradient without float atomics: split reductions go through ``ws`` (f32 tensor or None) and are summed in a fixed order;
    dW is overwritten."""
    call('yolo2_conv2d_wgrad_ws', ptr(X), ptr(dY), ptr(dW), ptr(ws), 0 if ws is None else ws.numel() * ws.element_size(), B, H, W, Cin, ldx, Cout, ldy,
         ksize, dtype_code(X.dtype), _stream())


def wgrad_ws_plan(B, H, W, Cin, ldx, Cout, ldy, ksize, dtype, cus):
    """Host plan of ``conv2d_wgrad_ws`` on a device with ``cus`` compute units: dict(family, slots, slot_floats, blocks)."""
    out = (ctypes.c_int * 4)()
    rc = _lib.load().yolo2_debug_wgrad_ws_plan(B, H, W, Cin, ldx, Cout, ldy, ksize, dtype_code(dtype), cus, out)
    if rc != 0:
        raise _lib.HipKernelError('yolo2_debug_wgrad_ws_plan failed (code %d)' % rc)
    return dict(zip(('family', 'slots', 'slot_floats', 'blocks'), list(out)))


def set_deterministic(on):
    """Deterministic mode of the calling thread (include/yolo2_hip.h yolo2_set_deterministic)."""
    call('yolo2_set_deterministic', 1 if on else 0)


class deterministic_launches(object):
    """``with ops.deterministic_launches(on):`` -- the calling thread's launch rules are the deterministic ones inside the block (when ``on``); on exit
    the thread's mode is what it was on entry (nested blocks, a caller that set the mode itself).  A default engine (``on`` false) never touches
    the library's switch."""

    def __init__(self, on):
        self.on = bool(on)
        self.prev = 0

    def __enter__(self):
        if self.on:
            self.prev = int(_lib.query('yolo2_get_deterministic'))
            if not self.prev:
                set_deterministic(True)

    def __exit__(self, *exc):
        if self.on and not self.prev:
            set_deterministic(False)
        return False


def filter_prep(Wt, Ffwd, Fdgr, ksize, Cin, ldcin, Cout, ldcout, dtype):
    call('yolo2_filter_prep', ptr(Wt), ptr(Ffwd), ptr(Fdgr), ksize, Cin, ldcin, Cout, ldcout, dtype_code(dtype), _stream())


def filter_prep_batch(descs_dev, n, total_blocks, dtype):
    call('yolo2_filter_prep_batch', ptr(descs_dev), n, total_blocks, dtype_code(dtype), _stream())


def adam_filter_prep(descs_dev, n, total_blocks, small_dev, n_small, params, grads, m, v, alpha, b1, b2, eps, gscale, dtype):
    call('yolo2_adam_filter_prep', ptr(descs_dev), n, total_blocks, ptr(small_dev), n_small, ptr(params), ptr(grads), ptr(m), ptr(v), alpha, b1, b2, eps, gscale,
         dtype_code(dtype), _stream())


def bn_stats(Y, mean, var, ws, M, C):
    call('yolo2_bn_stats', ptr(Y), ptr(mean), ptr(var), ptr(ws), M, C, dtype_code(Y.dtype), _stream())


def bn_stats_ema(Y, mean, var, mm, mv, decay, ws, M, C):
    call('yolo2_bn_stats_ema', ptr(Y), ptr(mean), ptr(var), ptr(mm), ptr(mv), decay, ptr(ws), M, C, dtype_code(Y.dtype), _stream())


def bn_ema(mm, mv, mean, var, C, decay):
    call('yolo2_bn_ema', ptr(mm), ptr(mv), ptr(mean), ptr(var), C, decay, _stream())


def bn_leaky(Y, mean, var, gamma, beta, A, M, C, lda, eps, alpha):
    call('yolo2_bn_leaky', ptr(Y), ptr(mean), ptr(var), ptr(gamma), ptr(beta), ptr(A), M, C, lda, eps, alpha, dtype_code(Y.dtype), _stream())


def bn_leaky_bwd_reduce(dA, ldda, Y, mean, var, gamma, beta, dgamma, dbeta, ws, M, C, eps, alpha):
    call('yolo2_bn_leaky_bwd_reduce', ptr(dA), ldda, ptr(Y), ptr(mean), ptr(var), ptr(gamma), ptr(beta), ptr(dgamma), ptr(dbeta), ptr(ws),
         M, C, eps, alpha, dtype_code(Y.dtype), _stream())


def bn_leaky_bwd_apply(dA, ldda, Y, mean, var, gamma, beta, dgamma, dbeta, dY, M, C, eps, alpha):
    call('yolo2_bn_leaky_bwd_apply', ptr(dA), ldda, ptr(Y), ptr(mean), ptr(var), ptr(gamma), ptr(beta), ptr(dgamma), ptr(dbeta), ptr(dY),
         M, C, eps, alpha, dtype_code(Y.dtype), _stream())


# ---- consumers that finalise the partial rows in their own prologue (include/yolo2_hip.h: yolo2_bn_leaky_fin & co.)
def last_bn_part_rows():
    """Partial rows used by this thread's most recent statistics-producing launch (conv2d_bn / conv2d_dgrad_bn)."""
    return int(_lib.load().yolo2_last_bn_part_rows())


def bn_fin_supported(rows, C, dtype):
    return bool(_lib.load().yolo2_bn_fin_supported(int(rows), int(C), dtype_code(dtype)))


def bn_fin_rows_limit(C, dtype, cap=1024):
    """Largest power-of-two partial-row count (<= cap) a *_fin consumer accepts for C channels; 0 if the shape never qualifies."""
    r = cap
    while r >= 1 and not bn_fin_supported(r, C, dtype):
        r //= 2
    return r


def _zero_args(zero, zero_floats):
    return (ptr(zero) if zero_floats else None), int(zero_floats)


def bn_leaky_fin(Y, bn_part, rows, shift, mean, var, mm, mv, decay, gamma, beta, A, M, C, lda, eps, alpha, zero=None, zero_floats=0):
    z, zn = _zero_args(zero, zero_floats)
    call('yolo2_bn_leaky_fin', ptr(Y), ptr(bn_part), rows, ptr(shift), ptr(mean), ptr(var), ptr(mm), ptr(mv), decay, ptr(gamma), ptr(beta), ptr(A),
         M, C, lda, eps, alpha, z, zn, dtype_code(Y.dtype), _stream())


def bn_leaky_pool_fin(Y, bn_part, rows, shift, mean, var, mm, mv, decay, gamma, beta, P, idx, B, H, W, C, ldp, eps, alpha, zero=None, zero_floats=0, ymax=None, a_full=None):
    z, zn = _zero_args(zero, zero_floats)
    call('yolo2_bn_leaky_pool_fin', ptr(Y), ptr(bn_part), rows, ptr(shift), ptr(mean), ptr(var), ptr(mm), ptr(mv), decay, ptr(gamma), ptr(beta),
         ptr(P), ptr(idx), ptr(ymax), ptr(a_full), B, H, W, C, ldp, eps, alpha, z, zn, dtype_code(Y.dtype), _stream())


def bn_leaky_bwd_apply_fin(dA, ldda, Y, mean, var, gamma, beta, part, rows, plane_stride, dgamma, dbeta, dY, M, C, eps, alpha, zero=None, zero_floats=0):
    z, zn = _zero_args(zero, zero_floats)
    call('yolo2_bn_leaky_bwd_apply_fin', ptr(dA), ldda, ptr(Y), ptr(mean), ptr(var), ptr(gamma), ptr(beta), ptr(part), rows, plane_stride,
         ptr(dgamma), ptr(dbeta), ptr(dY), M, C, eps, alpha, z, zn, dtype_code(Y.dtype), _stream())


def bn_leaky_pool_bwd_apply_fin(dP, lddp, idx, Y, mean, var, gamma, beta, part, rows, plane_stride, dgamma, dbeta, dY, B, H, W, C, eps, alpha,
                                zero=None, zero_floats=0):
    z, zn = _zero_args(zero, zero_floats)
    call('yolo2_bn_leaky_pool_bwd_apply_fin', ptr(dP), lddp, ptr(idx), ptr(Y), ptr(mean), ptr(var), ptr(gamma), ptr(beta), ptr(part), rows, plane_stride,
         ptr(dgamma), ptr(dbeta), ptr(dY), B, H, W, C, eps, alpha, z, zn, dtype_code(Y.dtype), _stream())


def first_layer_wgrad_bn(X, Y, dP, lddp, idx, mean, var, gamma, beta, part, rows, plane_stride, dgamma, dbeta, dW, B, H, W, Cin, eps, alpha,
                         zero=None, zero_floats=0):
    """Image layer: ``bn_leaky_pool_bwd_apply_fin`` + ``conv2d_wgrad`` in one launch (the layer's output gradient never reaches HBM)."""
    z, zn = _zero_args(zero, zero_floats)
    call('yolo2_first_layer_wgrad_bn', ptr(X), ptr(Y), ptr(dP), lddp, ptr(idx), ptr(mean), ptr(var), ptr(gamma), ptr(beta), ptr(part), rows, plane_stride,
         ptr(dgamma), ptr(dbeta), ptr(dW), B, H, W, Cin, eps, alpha, z, zn, dtype_code(Y.dtype), _stream())


def bn_leaky_bwd_reduce_part(dA, ldda, Y, mean, var, gamma, beta, ws, rows_limit, M, C, eps, alpha):
    """-> number of partial rows left in ``ws`` ([2][rows][C] f32)."""
    rows = ctypes.c_int(0)
    call('yolo2_bn_leaky_bwd_reduce_part', ptr(dA), ldda, ptr(Y), ptr(mean), ptr(var), ptr(gamma), ptr(beta), ptr(ws), ctypes.byref(rows), rows_limit, M, C,
         eps, alpha, dtype_code(Y.dtype), _stream())
    return rows.value


def bn_leaky_pool_bwd_reduce_part(dP, lddp, idx, Y, mean, var, gamma, beta, ws, rows_limit, B, H, W, C, eps, alpha):
    rows = ctypes.c_int(0)
    call('yolo2_bn_leaky_pool_bwd_reduce_part', ptr(dP), lddp, ptr(idx), ptr(Y), ptr(mean), ptr(var), ptr(gamma), ptr(beta), ptr(ws), ctypes.byref(rows),
         rows_limit, B, H, W, C, eps, alpha, dtype_code(Y.dtype), _stream())
    return rows.value


def bn_leaky_pool(Y, mean, var, gamma, beta, P, idx, B, H, W, C, ldp, eps, alpha):
    call('yolo2_bn_leaky_pool', ptr(Y), ptr(mean), ptr(var), ptr(gamma), ptr(beta), ptr(P), ptr(idx), B, H, W, C, ldp, eps, alpha,
         dtype_code(Y.dtype), _stream())


def bn_leaky_pool_bwd_reduce(dP, lddp, idx, Y, mean, var, gamma, beta, dgamma, dbeta, ws, B, H, W, C, eps, alpha):
    call('yolo2_bn_leaky_pool_bwd_reduce', ptr(dP), lddp, ptr(idx), ptr(Y), ptr(mean), ptr(var), ptr(gamma), ptr(beta), ptr(dgamma), ptr(dbeta),
         ptr(ws), B, H, W, C, eps, alpha, dtype_code(Y.dtype), _stream())


def bn_leaky_pool_bwd_apply(dP, lddp, idx, Y, mean, var, gamma, beta, dgamma, dbeta, dY, B, H, W, C, eps, alpha):
    call('yolo2_bn_leaky_pool_bwd_apply', ptr(dP), lddp, ptr(idx), ptr(Y), ptr(mean), ptr(var), ptr(gamma), ptr(beta), ptr(dgamma), ptr(dbeta),
         ptr(dY), B, H, W, C, eps, alpha, dtype_code(Y.dtype), _stream())


def maxpool_fwd(A, P, B, H, W, C, stride):
    call('yolo2_maxpool_fwd', ptr(A), ptr(P), B, H, W, C, stride, dtype_code(A.dtype), _stream())


def maxpool_bwd(A, dP, dA, B, H, W, C, stride):
    call('yolo2_maxpool_bwd', ptr(A), ptr(dP), ptr(dA), B, H, W, C, stride, dtype_code(A.dtype), _stream())


def maxpool_bwd_acc(A, dP, dA, B, H, W, C):
    call('yolo2_maxpool_bwd_acc', ptr(A), ptr(dP), ptr(dA), B, H, W, C, dtype_code(A.dtype), _stream())


def reorg(x, out, B, H, W, C, ldo):
    call('yolo2_reorg', ptr(x), ptr(out), B, H, W, C, ldo, dtype_code(x.dtype), _stream())


def reorg_bwd(dout, ldd, din, B, H, W, C):
    call('yolo2_reorg_bwd', ptr(dout), ldd, ptr(din), B, H, W, C, dtype_code(din.dtype), _stream())


def copy_channels(src, lds, dst, ldd, M, C):
    call('yolo2_copy_channels', ptr(src), lds, ptr(dst), ldd, M, C, dtype_code(src.dtype), _stream())


def add_inplace(dst, src, n):
    call('yolo2_add_inplace', ptr(dst), ptr(src), n, dtype_code(dst.dtype), _stream())


def bias_grad(dY, ld, dbias, ws, M, C):
    call('yolo2_bias_grad', ptr(dY), ld, ptr(dbias), ptr(ws), M, C, dtype_code(dY.dtype), _stream())


def image_prep(img, out, ws, B, HW, mode):
    call('yolo2_image_prep', ptr(img), ptr(out), ptr(ws), B, HW, mode, dtype_code(out.dtype), _stream())


def head_decode(logits, ld, anchors, conf, xy_min, xy_max, nan_flag, B, ch, cw, A, C):
    call('yolo2_head_decode', ptr(logits), ld, ptr(anchors), ptr(conf), ptr(xy_min), ptr(xy_max), ptr(nan_flag), B, ch, cw, A, C,
         dtype_code(logits.dtype), _stream())


def head_decode_attrs(logits, ld, anchors, iou, prob, xy, wh, B, ch, cw, A, C):
    call('yolo2_head_decode_attrs', ptr(logits), ld, ptr(anchors), ptr(iou), ptr(prob), ptr(xy), ptr(wh), B, ch, cw, A, C,
         dtype_code(logits.dtype), _stream())


def box_loss_code(box_loss):
    """'mse' | 'iou' | 'giou' | 'diou' | 'ciou' -> the int of yolo2_loss_box; anything else raises ValueError (host only)."""
    try:
        return _lib.BOX_LOSSES[box_loss]
    except (KeyError, TypeError):
        raise ValueError('box_loss = %r: one of %s' % (box_loss, ', '.join(_lib.BOX_LOSSES)))


def loss_options(box_loss='mse', class_loss='mse', ignore_thresh=0.0, rescore=False, label_smoothing=0.0, focal_gamma=2.0):
    """The options of the YOLOv2 loss (DESIGN.md sections 21 and 22) checked on the host: None when only ``box_loss`` may differ from its default
    (the call made before the other options existed serves), else the ``_lib.LossOptions`` of yolo2_loss_ex.  An unknown name or a value out of
    range raises ValueError naming the option."""
    mode = box_loss_code(box_loss)
    try:
        cls = _lib.CLASS_LOSSES[class_loss]
    except (KeyError, TypeError):
        raise ValueError('class_loss = %r: one of %s' % (class_loss, ', '.join(_lib.CLASS_LOSSES)))
    try:
        t, eps, gamma = float(ignore_thresh), float(label_smoothing), float(focal_gamma)
    except (TypeError, ValueError):
        raise ValueError('ignore_thresh, label_smoothing and focal_gamma are numbers, not %r, %r, %r' % (ignore_thresh, label_smoothing, focal_gamma))
    if not (t == 0.0 or 0.0 < t < 1.0):
        raise ValueError('ignore_thresh = %r: 0 (off) or a threshold inside (0, 1)' % (ignore_thresh,))
    if rescore not in (False, True, 0, 1):
        raise ValueError('rescore = %r: True or False' % (rescore,))
    if not 0.0 <= eps < 1.0:
        raise ValueError('label_smoothing = %r: lies in [0, 1)' % (label_smoothing,))
    if eps != 0.0 and cls == 0:
        raise ValueError('label_smoothing = %r with class_loss mse: smoothing belongs to ce and focal' % (label_smoothing,))
    if cls == 2 and not (gamma == 0.0 or (1.0 <= gamma < float('inf'))):
        raise ValueError('focal_gamma = %r: 0 or at least 1' % (focal_gamma,))
    if cls == 0 and t == 0.0 and not rescore:
        return None
    return _lib.LossOptions(ctypes.sizeof(_lib.LossOptions), mode, cls, int(bool(rescore)), t, eps, gamma if cls == 2 else 2.0)


def loss(logits, ld, anchors, labels, hparam, objectives, dlogits, ws, B, ch, cw, A, C, box_loss='mse', class_loss='mse', ignore_thresh=0.0,
         rescore=False, label_smoothing=0.0, focal_gamma=2.0):
    """labels: 6 device f32 tensors (mask, prob, coords, off_min, off_max, areas); hparam: 4 host floats
    in the order iou_best, iou_normal, coords, prob.  ``box_loss``: 'mse' (the reference's squared error, the call made before the option
    existed) or 'iou' / 'giou' / 'diou' / 'ciou' (DESIGN.md section 21).  ``class_loss`` 'mse' | 'ce' | 'focal' with ``label_smoothing`` and
    ``focal_gamma``, ``ignore_thresh`` and ``rescore``: DESIGN.md section 22; with all of them at their defaults the call is yolo2_loss or
    yolo2_loss_box as before, otherwise yolo2_loss_ex."""
    mode = box_loss_code(box_loss)
    opt = loss_options(box_loss, class_loss, ignore_thresh, rescore, label_smoothing, focal_gamma)
    hp = (ctypes.c_float * 4)(*[float(v) for v in hparam])
    mask, prob, coords, omin, omax, areas = labels
    if opt is not None:
        call('yolo2_loss_ex', ptr(logits), ld, ptr(anchors), ptr(mask), ptr(prob), ptr(coords), ptr(omin), ptr(omax), ptr(areas), hp,
             ptr(objectives), ptr(dlogits), ptr(ws), B, ch, cw, A, C, dtype_code(logits.dtype), _stream(), ctypes.byref(opt))
    elif mode == 0:
        call('yolo2_loss', ptr(logits), ld, ptr(anchors), ptr(mask), ptr(prob), ptr(coords), ptr(omin), ptr(omax), ptr(areas), hp,
             ptr(objectives), ptr(dlogits), ptr(ws), B, ch, cw, A, C, dtype_code(logits.dtype), _stream())
    else:
        call('yolo2_loss_box', ptr(logits), ld, ptr(anchors), ptr(mask), ptr(prob), ptr(coords), ptr(omin), ptr(omax), ptr(areas), hp,
             ptr(objectives), ptr(dlogits), ptr(ws), B, ch, cw, A, C, dtype_code(logits.dtype), _stream(), mode)


def loss_partials(logits, ld, anchors, labels, hparam, dlogits, ws, B, ch, cw, A, C, box_loss='mse', class_loss='mse', ignore_thresh=0.0,
                  rescore=False, label_smoothing=0.0, focal_gamma=2.0):
    """The loss kernel alone: dlogits + per-workgroup partial sums in ``ws``; ``loss_objectives`` reduces them on demand.  Options as in ``loss``."""
    mode = box_loss_code(box_loss)
    opt = loss_options(box_loss, class_loss, ignore_thresh, rescore, label_smoothing, focal_gamma)
    hp = (ctypes.c_float * 4)(*[float(v) for v in hparam])
    mask, prob, coords, omin, omax, areas = labels
    if opt is not None:
        call('yolo2_loss_ex_partials', ptr(logits), ld, ptr(anchors), ptr(mask), ptr(prob), ptr(coords), ptr(omin), ptr(omax), ptr(areas), hp,
             ptr(dlogits), ptr(ws), B, ch, cw, A, C, dtype_code(logits.dtype), _stream(), ctypes.byref(opt))
    elif mode == 0:
        call('yolo2_loss_partials', ptr(logits), ld, ptr(anchors), ptr(mask), ptr(prob), ptr(coords), ptr(omin), ptr(omax), ptr(areas), hp,
             ptr(dlogits), ptr(ws), B, ch, cw, A, C, dtype_code(logits.dtype), _stream())
    else:
        call('yolo2_loss_box_partials', ptr(logits), ld, ptr(anchors), ptr(mask), ptr(prob), ptr(coords), ptr(omin), ptr(omax), ptr(areas), hp,
             ptr(dlogits), ptr(ws), B, ch, cw, A, C, dtype_code(logits.dtype), _stream(), mode)


def loss_objectives(ws, objectives, B, ch, cw, A):
    call('yolo2_loss_objectives', ptr(ws), ptr(objectives), B, ch, cw, A, _stream())


def loss_ws_floats(B, cells, A):
    return workspace_bytes('loss', B, cells, A) // 4


def distill_options(weight=1.0, objectness=1.0, coords=1.0, prob=1.0, class_term='mse', temperature=1.0, scale_by_objectness=True):
    """The ``_lib.DistillOptions`` of yolo2_distill_partials, checked on the host: an unknown class term, a temperature
    that is not positive and finite, a negative or non-finite weight raise ValueError naming the option."""
    try:
        term = _lib.DISTILL_CLASS_TERMS[class_term]
    except (KeyError, TypeError):
        raise ValueError('class_term = %r: one of %s' % (class_term, ', '.join(_lib.DISTILL_CLASS_TERMS)))
    try:
        T = float(temperature)
        w = [float(v) for v in (weight, objectness, coords, prob)]
    except (TypeError, ValueError):
        raise ValueError('temperature and the distill weights are numbers, not %r, %r' % (temperature, (weight, objectness, coords, prob)))
    if not 0.0 < T < float('inf'):
        raise ValueError('temperature = %r: positive and finite' % (temperature,))
    for name, v in zip(('weight', 'objectness', 'coords', 'prob'), w):
        if not 0.0 <= v < float('inf'):
            raise ValueError('%s = %r: a weight >= 0' % (name, v))
    if scale_by_objectness not in (False, True, 0, 1):
        raise ValueError('scale_by_objectness = %r: True or False' % (scale_by_objectness,))
    return _lib.DistillOptions(ctypes.sizeof(_lib.DistillOptions), term, int(bool(scale_by_objectness)), w[0], w[1], w[2], w[3], T)


def distill_partials(student, ld_s, teacher, ld_t, dlogits, ws, B, ch, cw, A, C, **options):
    """The distill kernel alone: adds d(weighted distill term)/d student into ``dlogits`` (the student's dtype and ld; None: objectives only) and
    leaves per-workgroup partial sums in ``ws``; ``distill_objectives`` reduces them on demand.  ``student`` / ``teacher``: f32 or bf16 logits,
    each with its own ld; the two dtypes may differ.  Options as in ``distill_options``."""
    opt = distill_options(**options)
    call('yolo2_distill_partials', ptr(student), ld_s, dtype_code(student.dtype), ptr(teacher), ld_t, dtype_code(teacher.dtype), ptr(dlogits), ptr(ws),
         B, ch, cw, A, C, _stream(), ctypes.byref(opt))


def distill_objectives(ws, objectives, B, ch, cw, A):
    """objectives f32[3]: the unweighted objectness, coords and prob terms of the last ``distill_partials`` on ``ws``."""
    call('yolo2_distill_objectives', ptr(ws), ptr(objectives), B, ch, cw, A, _stream())


def distill_ws_floats(B, cells, A):
    return workspace_bytes('distill', B, cells, A) // 4


def nms(conf, xy_min, xy_max, order, ws, B, N, C, thr, thr_iou):
    call('yolo2_nms', ptr(conf), ptr(xy_min), ptr(xy_max), ptr(order), ptr(ws), B, N, C, thr, thr_iou, _stream())


def soft_nms(conf, xy_min, xy_max, order, B, N, C, method, thr, thr_iou, sigma=0.5):
    """yolo2_soft_nms: method 'hard', 'linear' or 'gaussian' (or its YOLO2_NMS_* code); order may be None."""
    if isinstance(method, str):
        if method not in _lib.NMS_METHODS:
            raise ValueError('nms method must be one of %s, not %r' % (', '.join(_lib.NMS_METHODS), method))
        method = _lib.NMS_METHODS[method]
    call('yolo2_soft_nms', ptr(conf), ptr(xy_min), ptr(xy_max), ptr(order), B, N, C, int(method), thr, thr_iou, sigma, _stream())


def tta_gather(conf, xy_min, xy_max, out_conf, out_xy_min, out_xy_max, B, N, C, M, offset, sx, sy, cell_w0, flip):
    """yolo2_tta_gather: one view's boxes -> rows offset .. offset+N-1 of the pooled [B,M,.] buffers, in the base grid (sx, sy: f32 scales)."""
    call('yolo2_tta_gather', ptr(conf), ptr(xy_min), ptr(xy_max), ptr(out_conf), ptr(out_xy_min), ptr(out_xy_max), B, N, C, M, int(offset),
         float(sx), float(sy), float(cell_w0), int(bool(flip)), _stream())


def wbf(conf, xy_min, xy_max, out_conf, out_xy_min, out_xy_max, rows, flags, ws, B, M, C, V, max_per_class, R, thr, fuse_iou):
    """yolo2_wbf: Weighted Boxes Fusion of the pooled boxes per (image, class); ws: ``workspace_bytes('wbf', B, C, max_per_class)`` bytes;
    flags (one int32, zeroed by the caller) is OR-ed with the WBF_FLAG_* overflow bits."""
    call('yolo2_wbf', ptr(conf), ptr(xy_min), ptr(xy_max), ptr(out_conf), ptr(out_xy_min), ptr(out_xy_max), ptr(rows), ptr(flags), ptr(ws),
         B, M, C, int(V), int(max_per_class), int(R), float(thr), float(fuse_iou), _stream())


WBF_MAX_CANDIDATES = 4096                                               # YOLO2_WBF_MAX_CANDIDATES
WBF_FLAG_CANDIDATES, WBF_FLAG_CLUSTERS, WBF_FLAG_ROWS = 1, 2, 4        # YOLO2_WBF_FLAG_*


def adam(w, g, m, v, n, alpha, b1, b2, eps, gscale=1.0):
    call('yolo2_adam', ptr(w), ptr(g), ptr(m), ptr(v), n, alpha, b1, b2, eps, gscale, _stream())


def momentum(w, g, acc, n, lr, mom, gscale=1.0):
    call('yolo2_momentum', ptr(w), ptr(g), ptr(acc), n, lr, mom, gscale, _stream())


def sgd(w, g, n, lr, gscale=1.0):
    call('yolo2_sgd', ptr(w), ptr(g), n, lr, gscale, _stream())


def rmsprop(w, g, ms, mom, n, lr, decay, momentum_, eps, gscale=1.0):
    call('yolo2_rmsprop', ptr(w), ptr(g), ptr(ms), ptr(mom), n, lr, decay, momentum_, eps, gscale, _stream())


def adagrad(w, g, acc, n, lr, gscale=1.0):
    call('yolo2_adagrad', ptr(w), ptr(g), ptr(acc), n, lr, gscale, _stream())


def adadelta(w, g, acc, accu, n, lr, rho, eps, gscale=1.0):
    call('yolo2_adadelta', ptr(w), ptr(g), ptr(acc), ptr(accu), n, lr, rho, eps, gscale, _stream())


def ftrl(w, g, accum, linear, n, lr, lr_power, l1, l2, gscale=1.0):
    call('yolo2_ftrl', ptr(w), ptr(g), ptr(accum), ptr(linear), n, lr, lr_power, l1, l2, gscale, _stream())


def scale(x, n, s):
    call('yolo2_scale', ptr(x), n, s, _stream())


def ema_update(ema, w, n, one_minus_decay):
    """ema -= (ema - w) * one_minus_decay over ``n`` f32 elements (tf.train.ExponentialMovingAverage's assign_moving_average), one launch."""
    call('yolo2_ema_update', ptr(ema), ptr(w), n, one_minus_decay, _stream())


GRAD_STORE, GRAD_ADD, GRAD_FINAL = 0, 1, 2           # YOLO2_GRAD_*: mode of yolo2_grad_combine
GRAD_COMBINE_CHUNK = 4096                            # YOLO2_GRAD_COMBINE_CHUNK: elements of one workgroup's chunk


def check_grad_ranges(ranges, n):
    """``ranges`` as a list of (begin, end) ints after checking what yolo2_grad_combine relies on: 0 <= begin < end <= n, sorted, disjoint
    (adjacent ranges are fine).  Raises ValueError otherwise.  Pure host logic."""
    out, last = [], 0
    for b, e in ranges:
        b, e = int(b), int(e)
        if not (0 <= b < e <= n):
            raise ValueError('grad_combine: the range [%d, %d) is empty or outside [0, %d)' % (b, e, n))
        if b < last:
            raise ValueError('grad_combine: the range [%d, %d) is out of order or overlaps the range before it (which ends at %d)' % (b, e, last))
        out.append((b, e))
        last = e
    return out


def grad_ranges(ranges, n, device):
    """The device table of yolo2_grad_combine for ``ranges`` (checked by ``check_grad_ranges``): int64 [2 * len(ranges)], or None when there is none."""
    flat = [v for be in check_grad_ranges(ranges, n) for v in be]
    return torch.tensor(flat, dtype=torch.int64, device=device) if flat else None


def grad_combine(g, acc, w, n, mode, scale=1.0, decay=0.0, shrink=1.0, table=None):
    """One launch over ``n`` f32 elements (include/yolo2_hip.h yolo2_grad_combine): GRAD_STORE acc = g; GRAD_ADD acc += g; GRAD_FINAL
    g = (acc + g) * scale (+ decay * w inside the table's ranges), w *= shrink inside them.  ``table``: what ``grad_ranges`` returned."""
    call('yolo2_grad_combine', ptr(g), ptr(acc), ptr(w), n, mode, scale, decay, shrink, ptr(table), 0 if table is None else table.numel() // 2, _stream())


def zero_ranges(x, ranges):
    """x[a:b] = 0 for every (a, b) in ``ranges`` (element offsets; host list)."""
    flat = (ctypes.c_long * (2 * len(ranges)))(*[int(v) for ab in ranges for v in ab])
    call('yolo2_zero_ranges', ptr(x), flat, len(ranges), _stream())


def bn_fold(W, gamma, beta, mean, var, Wf, bias, rows, C, eps):
    call('yolo2_bn_fold', ptr(W), ptr(gamma), ptr(beta), ptr(mean), ptr(var), ptr(Wf), ptr(bias), rows, C, eps, _stream())


def workspace_bytes(kind, *args):
    """Caller-owned scratch size of an entry family: 'conv2d', 'bn', 'bias_grad', 'image_prep', 'loss', 'distill', 'nms', 'wbf', 'clip', 'augment'
    (include/yolo2_hip.h yolo2_*_workspace_bytes)."""
    return int(_lib.query('yolo2_%s_workspace_bytes' % kind, *args))


def clip_by_norm(g, seg_off, nseg, clip, ws):
    call('yolo2_clip_by_norm', ptr(g), ptr(seg_off), nseg, clip, ptr(ws), _stream())


def clip_by_norm_fixed(g, seg_off, nseg, clip, ws):
    """Per-tensor clip with fixed-order sums of squares (deterministic mode); ws: f64 tensor of ``workspace_bytes('clip_fixed', nseg)`` bytes."""
    call('yolo2_clip_by_norm_fixed', ptr(g), ptr(seg_off), nseg, clip, ptr(ws), ws.numel() * ws.element_size(), _stream())


def selftest_tr16():
    out = torch.zeros(256, dtype=torch.int16, device='cuda')
    call('yolo2_selftest_tr16', ptr(out), _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(64, 4)


CONV_PLAN_KEYS = ('BM', 'BN', 'waves', 'chunks', 'stages', 'split', 'grid_x', 'grid_y')
WGRAD_PLAN_KEYS = ('BC', 'BN', 'waves', 'pair', 'ranges', 'remap', 'blocks', 'direct')


def last_conv_plan():
    """Variant of this thread's most recent conv2d* launch (include/yolo2_hip.h yolo2_debug_last_conv_plan)."""
    out = (ctypes.c_int * 8)()
    _lib.load().yolo2_debug_last_conv_plan(out)
    return dict(zip(CONV_PLAN_KEYS, list(out)))


CONV_ROUTE_MODES = {'plain': 0, 'bias_act': 1, 'bn': 2, 'dgrad_bn': 3}
CONV_ROUTE_EXCLUDE = {'first': 1, 'c32': 2, 'c64': 4, 'd1': 8, 'tap': 16, 's4': 32, 'stream': 64}
CONV_ROUTE_STATS = ('none', 'epilogue', 'colsum', 'two_step')
CONV_ROUTE_FAMILIES = ('first', 'c32', 'c64', 'd1', 'pp', 's4', 'igemm')


def conv_route(B, H, W, Cp, ldp, Nf, ldo, ksize, dtype, mode, ws_bytes, cus=0, exclude=(), align_bits=7):
    """Host-side route of a conv2d* call (include/yolo2_hip.h yolo2_debug_conv_route; no device): dict(plan, rows, stats, pending, family).
    ``mode``: a key of CONV_ROUTE_MODES; ``exclude``: keys of CONV_ROUTE_EXCLUDE; ``cus`` 0: the process's current workgroup count."""
    out = (ctypes.c_int * 12)()
    mask = 0
    for name in exclude:
        mask |= CONV_ROUTE_EXCLUDE[name]
    rc = _lib.load().yolo2_debug_conv_route(B, H, W, Cp, ldp, Nf, ldo, ksize, dtype_code(dtype), CONV_ROUTE_MODES[mode], align_bits, ws_bytes, cus, mask, out)
    if rc != 0:
        raise _lib.HipKernelError('yolo2_debug_conv_route failed (code %d)' % rc)
    return dict(plan=dict(zip(CONV_PLAN_KEYS, list(out)[:8])), rows=out[8], stats=CONV_ROUTE_STATS[out[9]], pending=out[10], family=CONV_ROUTE_FAMILIES[out[11]])


def noop():
    """Empty kernel on the current stream (event-bracket calibration in bench.py)."""
    call('yolo2_debug_noop', _stream())


def set_igemm_tap(mode):
    """Test hook (process-wide): 0 = per-tap 3x3 kernels only, non-zero = the ping-pong tap-fused kernel where its launch rule admits it (default)."""
    _lib.load().yolo2_debug_set_igemm_tap(int(mode))


def set_pp(grid=-1, dmapos=-1, min_steps=-1, min_share=-1):
    """Test / A-B hook for the ping-pong kernel (include/yolo2_hip.h yolo2_debug_set_pp); negative = keep."""
    _lib.load().yolo2_debug_set_pp(int(grid), int(dmapos), int(min_steps), int(min_share))


def set_pp_cost(cv):
    """Owner cost (K steps) of the ping-pong kernel's cost-balanced stream-K partition (yolo2_debug_set_pp_cost); 0 = equal K-step shares."""
    lib = _lib.load()
    if 'yolo2_debug_set_pp_cost' not in _lib.MISSING:
        lib.yolo2_debug_set_pp_cost(int(cv))


def check_async_errors():
    """Synchronises the current stream; raises RuntimeError when a stream-K tile owner gave up waiting for a partner (include/yolo2_hip.h
    yolo2_check_async_errors): errors surface, the device never hangs."""
    call('yolo2_check_async_errors', _stream())


class AsyncErrorPoll(object):
    """yolo2_async_error_snapshot without a synchronisation: ``snapshot()`` enqueues the 32-byte copy of the device's give-up counters into
    pinned host memory behind the work already on the current stream; ``pending()`` says whether a COMPLETED snapshot shows a failure (then
    ``check_async_errors()`` raises with the library's message and resets the pool).  One step of latency instead of one summary interval."""

    def __init__(self):
        self.words = torch.zeros(8, dtype=torch.int32).pin_memory()
        self.event = None

    def snapshot(self):
        _lib.load()
        if 'yolo2_async_error_snapshot' in _lib.MISSING:      # an earlier round's library in a same-box A/B (YOLO2_LIB_BASELINE=1)
            return
        call('yolo2_async_error_snapshot', self.words.data_ptr(), _stream())
        self.event = torch.cuda.Event()
        self.event.record()

    def pending(self):
        return self.event is not None and self.event.query() and bool(self.words.any().item())

    def raise_if_pending(self):
        if self.pending():
            self.event = None
            check_async_errors()
            raise RuntimeError('stream-K hand-off gave up (reported by yolo2_async_error_snapshot); convolution outputs since the last check are invalid')


def set_streamk_wait_us(us=0, unclamped=False):
    """Test hook: wait limit of the stream-K owners (0 = default 2 s) and the grid <= K-steps clamp."""
    call('yolo2_debug_set_streamk_wait_us', int(us), int(bool(unclamped)))


def last_wgrad_plan():
    out = (ctypes.c_int * 8)()
    _lib.load().yolo2_debug_last_wgrad_plan(out)
    return dict(zip(WGRAD_PLAN_KEYS, list(out)))


def set_wgrad_variant(v):
    _lib.load().yolo2_debug_set_wgrad_variant(int(v))


def augment_images(src, params_dev, ws, out, B, H, W, any_contrast):
    call('yolo2_augment_images', ptr(src), ptr(params_dev), ptr(ws), ptr(out), B, H, W, int(bool(any_contrast)), _stream())


def compose_images(src, tiles_dev, photo_dev, mix_dev, ws, out, B, L, T, H, W, fill, any_contrast):
    """Mosaic / MixUp: tiles_dev = the bytes of [B][L][T] ComposeTile, photo_dev of [B] AugmentParams, mix_dev of [B] f32 (None with L = 1)."""
    call('yolo2_compose_images', ptr(src), ptr(tiles_dev), ptr(photo_dev), ptr(mix_dev), ptr(ws), ptr(out), B, L, T, H, W, float(fill), int(bool(any_contrast)), _stream())


def transform_labels(objects_class, objects_coord, first_object, mask, prob, coords, offset_xy_min, offset_xy_max, areas, B, classes,
                     cell_width, cell_height, error_flag):
    call('yolo2_transform_labels', ptr(objects_class), ptr(objects_coord), ptr(first_object), ptr(mask), ptr(prob), ptr(coords),
         ptr(offset_xy_min), ptr(offset_xy_max), ptr(areas), B, classes, cell_width, cell_height, ptr(error_flag), _stream())


# ---- YOLO (v1) family
def yolo1_loss(net, ld, labels, hparam, objectives, dnet, ws, B, ch, cw, boxes, C):
    hp = (ctypes.c_float * 4)(*[float(v) for v in hparam])
    mask, prob, coords, omin, omax, areas = labels
    call('yolo1_loss', ptr(net), ld, ptr(mask), ptr(prob), ptr(coords), ptr(omin), ptr(omax), ptr(areas), hp, ptr(objectives), ptr(dnet), ptr(ws),
         B, ch, cw, boxes, C, dtype_code(net.dtype), _stream())


def yolo1_head_decode(net, ld, conf, xy_min, xy_max, nan_flag, B, ch, cw, boxes, C):
    call('yolo1_head_decode', ptr(net), ld, ptr(conf), ptr(xy_min), ptr(xy_max), ptr(nan_flag), B, ch, cw, boxes, C, dtype_code(net.dtype), _stream())


def leaky_bwd(A, dA, dZ, n, alpha):
    call('yolo2_leaky_bwd', ptr(A), ptr(dA), ptr(dZ), n, alpha, dtype_code(A.dtype), _stream())


def dropout(X, Y, mask, n, keep_prob, seed):
    call('yolo2_dropout', ptr(X), ptr(Y), ptr(mask), n, keep_prob, int(seed), dtype_code(X.dtype), _stream())


def dropout_bwd(dY, mask, dX, n, keep_prob):
    call('yolo2_dropout_bwd', ptr(dY), ptr(mask), ptr(dX), n, keep_prob, dtype_code(dY.dtype), _stream())


def l2_regularizer(w, g, n, scale, loss):
    call('yolo2_l2_regularizer', ptr(w), ptr(g), n, scale, ptr(loss), _stream())


# ---- image layer fused with its consumers (include/yolo2_hip.h: yolo2_first_layer_*)
def first_layer_stats(P, F, B, H, W, shift, bn_part):
    call('yolo2_first_layer_stats', ptr(P), ptr(F), B, H, W, ptr(shift), ptr(bn_part), dtype_code(P.dtype), _stream())


def first_layer_bn_leaky_pool(P, F, mean, var, gamma, beta, Pout, idx, B, H, W, ldp, eps, alpha):
    call('yolo2_first_layer_bn_leaky_pool', ptr(P), ptr(F), ptr(mean), ptr(var), ptr(gamma), ptr(beta), ptr(Pout), ptr(idx), B, H, W, ldp, eps, alpha,
         dtype_code(P.dtype), _stream())


def first_layer_pool_bwd_reduce(P, F, dP, lddp, idx, mean, var, gamma, beta, bn_part, B, H, W, eps, alpha):
    call('yolo2_first_layer_pool_bwd_reduce', ptr(P), ptr(F), ptr(dP), lddp, ptr(idx), ptr(mean), ptr(var), ptr(gamma), ptr(beta), ptr(bn_part), B, H, W,
         eps, alpha, dtype_code(P.dtype), _stream())


def first_layer_pool_bwd_apply(P, F, dP, lddp, idx, mean, var, gamma, beta, dgamma, dbeta, dY, B, H, W, eps, alpha):
    call('yolo2_first_layer_pool_bwd_apply', ptr(P), ptr(F), ptr(dP), lddp, ptr(idx), ptr(mean), ptr(var), ptr(gamma), ptr(beta), ptr(dgamma), ptr(dbeta),
         ptr(dY), B, H, W, eps, alpha, dtype_code(P.dtype), _stream())


# ---- data-parallel support
def set_stream_workgroups(n):
    """Stream-K convolution launches use ``n`` workgroups instead of one per CU (0 = default)."""
    call('yolo2_set_stream_workgroups', int(n))


def get_stream_workgroups():
    return int(_lib.load().yolo2_get_stream_workgroups())


def cast_f32_bf16(src, dst, n):
    call('yolo2_cast_f32_bf16', ptr(src), ptr(dst), n, _stream())


def cast_bf16_f32(src, dst, n):
    call('yolo2_cast_bf16_f32', ptr(src), ptr(dst), n, _stream())


def debug_occupy(workgroups, stop, started, max_us):
    call('yolo2_debug_occupy', workgroups, ptr(stop), ptr(started), max_us, _stream())


EVAL_MODES = {'detect': 0, 'all': 1}       # YOLO2_EVAL_MODE_* (include/yolo2_hip.h)
EVAL_RECORD_BYTES = 16                     # sizeof(yolo2_eval_record): score f32, image i32, box i32, class << 2 | flag
EVAL_STATE_WORDS = 2                       # YOLO2_EVAL_STATE_WORDS


def eval_collect(conf, xy_min, xy_max, gt_class, gt_box, gt_difficult, gt_first, G, B, N, C, n_valid, image_base, mode, threshold, iou_threshold,
                 records, max_records, state, npos, ws):
    """Stage A of the evaluator (yolo2_eval_collect): appends this batch's detection records and ground truth counts; asynchronous."""
    call('yolo2_eval_collect', ptr(conf), ptr(xy_min), ptr(xy_max), ptr(gt_class), ptr(gt_box), ptr(gt_difficult), ptr(gt_first), G, B, N, C,
         n_valid, image_base, mode, threshold, iou_threshold, ptr(records), max_records, ptr(state), ptr(npos), ptr(ws), _stream())


def eval_finalize(records, max_records, state, npos, C, n_images, N, ws, results, sorted_records=None, cum_tp=None, cum_fp=None):
    """Stage B of the evaluator (yolo2_eval_finalize): device sort per class + both VOC average precisions into ``results``; asynchronous."""
    call('yolo2_eval_finalize', ptr(records), max_records, ptr(state), ptr(npos), C, n_images, N, ptr(ws), ws.numel() * ws.element_size(),
         ptr(results), ptr(sorted_records), ptr(cum_tp), ptr(cum_fp), _stream())


# COCO protocol (include/yolo2_hip.h, section "evaluation, COCO protocol")
def _host(a, dtype):
    """A host table as (pointer or None, the array that keeps it alive): the library reads it during the call."""
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype)
    return a.ctypes.data, a


def eval_coco_collect(conf, xy_min, xy_max, gt_class, gt_box, gt_area, gt_flags, gt_first, scale, G, B, N, C, n_valid, image_base, mode, threshold,
                      area_ranges, A, iou_thresholds, T, max_dets, records, max_records, state, npig, ws):
    """Stage A of the COCO evaluator (yolo2_eval_coco_collect): greedy matching per (area range, IoU threshold) and the records of
    this batch; asynchronous.  area_ranges [A,2] f32 and iou_thresholds [T] f32 are HOST arrays."""
    pa, _ka = _host(area_ranges, np.float32)
    pt, _kt = _host(iou_thresholds, np.float32)
    call('yolo2_eval_coco_collect', ptr(conf), ptr(xy_min), ptr(xy_max), ptr(gt_class), ptr(gt_box), ptr(gt_area), ptr(gt_flags), ptr(gt_first),
         ptr(scale), G, B, N, C, n_valid, image_base, mode, threshold, pa, A, pt, T, max_dets, ptr(records), max_records, ptr(state), ptr(npig),
         ptr(ws), 0 if ws is None else ws.numel() * ws.element_size(), _stream())


def eval_coco_finalize(records, max_records, state, npig, C, n_images, N, A, T, max_dets, slices, S, recall_thresholds, R, ws, results):
    """Stage B of the COCO evaluator (yolo2_eval_coco_finalize): device sort + AP / recall per (slice, threshold, class) into
    ``results``; asynchronous.  slices [S,2] int32 and recall_thresholds [R] f64 are HOST arrays."""
    ps, _ks = _host(slices, np.int32)
    pr, _kr = _host(recall_thresholds, np.float64)
    call('yolo2_eval_coco_finalize', ptr(records), max_records, ptr(state), ptr(npig), C, n_images, N, A, T, max_dets, ps, S, pr, R, ptr(ws),
         0 if ws is None else ws.numel() * ws.element_size(), ptr(results), _stream())


# dimension clusters (include/yolo2_hip.h, section "dimension clusters")
ANCHOR_MAX_K = 32                          # YOLO2_ANCHOR_MAX_K
ANCHOR_MAX_JOBS = 65535                    # YOLO2_ANCHOR_MAX_JOBS
ANCHOR_MAX_BOXES = (1 << 27) - 1           # YOLO2_ANCHOR_MAX_BOXES


def anchor_assign(boxes, n, centroids, job_k, jobs, kmax, ws, done=None, assignment=None):
    """yolo2_anchor_assign: every box's best centroid (IoU of (w, h)) of every job, summed into the integer workspace; asynchronous."""
    call('yolo2_anchor_assign', ptr(boxes), n, ptr(centroids), ptr(job_k), jobs, kmax, ptr(ws), 0 if ws is None else ws.numel() * ws.element_size(),
         ptr(done), ptr(assignment), _stream())


def anchor_update(centroids, job_k, jobs, kmax, ws, n, done=None, iterations=None, counts=None, avg_iou=None):
    """yolo2_anchor_update: with ``done`` and ``iterations`` the Lloyd update (new centroids, fixed point detection); without both the
    score pass (centroids stay).  Either writes ``counts`` / ``avg_iou`` when given and clears the workspace; asynchronous."""
    call('yolo2_anchor_update', ptr(centroids), ptr(job_k), jobs, kmax, ptr(ws), 0 if ws is None else ws.numel() * ws.element_size(), n,
         ptr(done), ptr(iterations), ptr(counts), ptr(avg_iou), _stream())


HIST_BUCKETS = 1550        # YOLO2_HIST_BUCKETS / YOLO2_HIST_WORDS of include/yolo2_hip.h
HIST_WORDS = HIST_BUCKETS + 6


class HistogramJobs(object):
    """Device job table of yolo2_histogram, built once for a fixed list of tensors, with its result and workspace buffers.

    ``jobs``: [(tensor, rows, c, ld)] -- ``tensor`` a contiguous f32 / bf16 device tensor (a view is fine: its data_ptr() is the job's base) of
    which the job reads ``rows`` rows of ``c`` values with row stride ``ld``; (t, 1, n, n) is a flat range, rows = 0 an empty job.  The
    extents are checked against the tensors here, so the kernel never reads past one.  The tensors are kept alive by this object."""

    def __init__(self, jobs, device=None):
        from ._lib import HistJob
        assert len(jobs) > 0
        self.tensors = [j[0] for j in jobs]
        self.shapes = [(int(j[1]), int(j[2]), int(j[3])) for j in jobs]
        self.device = device if device is not None else self.tensors[0].device
        arr = (HistJob * len(jobs))()
        first = 0
        for d, (t, rows, c, ld) in zip(arr, jobs):
            rows, c, ld = int(rows), int(c), int(ld)
            assert t.is_cuda and t.is_contiguous() and 0 <= c <= ld and rows >= 0, (rows, c, ld)
            extent = (rows - 1) * ld + c if rows > 0 and c > 0 else 0
            assert extent <= t.numel(), 'histogram job of %d elements on a tensor of %d' % (extent, t.numel())
            if extent == 0:
                rows, c, ld = 0, 0, 0
            d.base, d.rows, d.c, d.ld, d.dtype, d.first_item = (t.data_ptr() if extent else None), rows, c, ld, dtype_code(t.dtype), first
            first += int(_lib.query('yolo2_histogram_items', rows, c, ld, d.dtype))
        self.n, self.items = len(jobs), first
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
        self.out = torch.zeros(self.n, HIST_WORDS, dtype=torch.int64, device=self.device)
        self.ws = torch.empty(max(workspace_bytes('histogram', self.n) // 8, 1), dtype=torch.int64, device=self.device)

    def launch(self):
        """Enqueues the call on the current stream (no synchronisation); the records are in ``self.out`` [n][HIST_WORDS] once it has run."""
        call('yolo2_histogram', ptr(self.table), self.n, self.items, ptr(self.out), self.out.numel() * 8, ptr(self.ws), self.ws.numel() * 8, _stream())
        return self.out


def decode_histograms(words):
    """Host view of yolo2_histogram's records: ``words`` an int64 array [n][HIST_WORDS] (numpy).  -> list of dicts with counts (int64 [1550]),
    min, max, sum, sum_squares (float), num, nonfinite (int)."""
    words = np.ascontiguousarray(words).reshape(-1, HIST_WORDS)
    out = []
    for w in words:
        stats = w[HIST_BUCKETS:HIST_BUCKETS + 4].view(np.float64)
        out.append({'counts': w[:HIST_BUCKETS], 'min': float(stats[0]), 'max': float(stats[1]), 'sum': float(stats[2]), 'sum_squares': float(stats[3]),
                    'num': int(w[HIST_BUCKETS + 4]), 'nonfinite': int(w[HIST_BUCKETS + 5])})
    return out


IMAGE_RECORD_BYTES = 16    # YOLO2_IMAGE_RECORD_BYTES of include/yolo2_hip.h


def image_depth(c):
    """Channels of the image yolo2_image_summary makes from ``c``: c for 1, 3, 4, otherwise 1 (the channel sum)."""
    return int(_lib.query('yolo2_image_summary_depth', int(c)))


class ImageJobs(object):
    """Device job table of yolo2_image_summary, built once for a fixed list of images, with its result and workspace buffers.

    ``jobs``: [(tensor, rows, c, ld)] -- one IMAGE each: ``tensor`` a contiguous f32 / bf16 device tensor (a view is fine: its data_ptr() is the
    job's base) of which the job reads ``rows`` = H*W pixels of ``c`` values every ``ld`` elements; rows = 0 is an empty job.  The extents are
    checked against the tensors here, so the kernel never reads past one.  The result is ONE uint8 buffer ``out``: the records, then every
    job's packed [rows][depth] bytes at ``offsets[j]`` (16-byte aligned).  The tensors are kept alive by this object."""

    def __init__(self, jobs, device=None):
        from ._lib import ImageJob
        assert len(jobs) > 0
        self.tensors = [j[0] for j in jobs]
        self.device = device if device is not None else self.tensors[0].device
        self.n = len(jobs)
        arr = (ImageJob * self.n)()
        first, sums, off = 0, 0, self.n * IMAGE_RECORD_BYTES
        self.inputs, self.shapes, self.offsets = [], [], []         # (rows, c, ld) read / (rows, depth) written / byte offset in out
        for d, (t, rows, c, ld) in zip(arr, jobs):
            rows, c, ld = int(rows), int(c), int(ld)
            assert t.is_cuda and t.is_contiguous() and 0 <= c <= ld and 0 <= rows < 2 ** 31, (rows, c, ld)
            extent = (rows - 1) * ld + c if rows > 0 and c > 0 else 0
            assert extent <= t.numel(), 'image job of %d elements on a tensor of %d' % (extent, t.numel())
            if extent == 0:
                rows, c, ld = 0, 0, 0
            depth = image_depth(c)
            summed = c > 0 and depth != c
            d.base, d.rows, d.c, d.ld, d.dtype, d.first_item = (t.data_ptr() if extent else None), rows, c, ld, dtype_code(t.dtype), first
            d.out_offset, d.sum_offset = off, (sums if summed else 0)
            self.inputs.append((rows, c, ld))
            self.shapes.append((rows, depth))
            self.offsets.append(off)
            first += int(_lib.query('yolo2_image_summary_items', rows, c, ld, d.dtype))
            sums += rows if summed else 0
            off += (rows * depth + 15) // 16 * 16
        self.items = first
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
        nbytes = int(_lib.query('yolo2_image_summary_result_bytes', self.n, off - self.n * IMAGE_RECORD_BYTES))
        assert nbytes == off
        self.out = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self.ws = torch.empty(max(int(_lib.query('yolo2_image_summary_workspace_bytes', self.n, sums)) // 4, 1), dtype=torch.int32, device=self.device)

    def launch(self):
        """Enqueues the call on the current stream (no synchronisation); records and images are in ``self.out`` once it has run."""
        call('yolo2_image_summary', ptr(self.table), self.n, self.items, ptr(self.out), self.out.numel(), ptr(self.ws), self.ws.numel() * 4, _stream())
        return self.out


def decode_images(buf, shapes, offsets):
    """Host view of yolo2_image_summary's result: ``buf`` a uint8 array (numpy) as ImageJobs.out, ``shapes`` / ``offsets`` of the same table.
    -> [(record dict with min, max, scale (float) and nonfinite (int), uint8 array [rows][depth])]."""
    buf = np.ascontiguousarray(buf)
    n = len(shapes)
    rec = buf[:n * IMAGE_RECORD_BYTES].view(np.uint32).reshape(n, 4)
    f = rec.view(np.float32)
    out = []
    for j, ((rows, depth), off) in enumerate(zip(shapes, offsets)):
        out.append(({'min': float(f[j, 0]), 'max': float(f[j, 1]), 'nonfinite': int(rec[j, 2]), 'scale': float(f[j, 3])},
                    buf[off:off + rows * depth].reshape(rows, depth)))
    return out


# ---- int8 inference (include/yolo2_hip.h "int8 inference"; specification: tests/quant_ref.py) ----------------------------------------

I8_OUT_I8, I8_OUT_BF16, I8_OUT_F32, I8_OUT_ACC = _lib.I8_OUT_I8, _lib.I8_OUT_BF16, _lib.I8_OUT_F32, _lib.I8_OUT_ACC


def conv2d_i8(P, F, mult, bias, O, B, H, W, Cp, ldp, Nf, ldo, ksize, alpha, inv_s_out, out_kind):
    """yolo2_conv2d_i8: int8 P / F, int32 accumulation, epilogue t = acc*mult, y = t + bias, leaky (alpha == 1: linear), then ``out_kind``:
    int8 clip(rint(y * inv_s_out)), bf16, f32, or the raw int32 accumulators (I8_OUT_ACC: mult / bias may be None)."""
    call('yolo2_conv2d_i8', ptr(P), ptr(F), ptr(mult), ptr(bias), ptr(O), B, H, W, Cp, ldp, Nf, ldo, ksize, float(alpha), float(inv_s_out), out_kind, _stream())


class AbsmaxJobs(object):
    """Device job table of yolo2_absmax over a fixed list of tensors, with its running result.

    ``jobs``: [(tensor, rows, c, ld, slot)] -- as HistogramJobs, plus the record the job folds into (several jobs may share one).  ``launch()``
    folds the tensors' current contents into the running records; ``result()`` -> (abs-max f32 [nslots], non-finite counts int64 [nslots])."""

    def __init__(self, jobs, nslots, device=None):
        from ._lib import AbsmaxJob
        assert len(jobs) > 0
        self.tensors = [j[0] for j in jobs]
        self.device = device if device is not None else self.tensors[0].device
        arr = (AbsmaxJob * len(jobs))()
        for d, (t, rows, c, ld, slot) in zip(arr, jobs):
            rows, c, ld, slot = int(rows), int(c), int(ld), int(slot)
            assert t.is_cuda and t.is_contiguous() and 0 < c <= ld and rows > 0 and 0 <= slot < nslots, (rows, c, ld, slot)
            assert (rows - 1) * ld + c <= t.numel(), 'abs-max job of %d elements on a tensor of %d' % ((rows - 1) * ld + c, t.numel())
            d.base, d.rows, d.c, d.ld, d.dtype, d.slot = t.data_ptr(), rows, c, ld, dtype_code(t.dtype), slot
        self.n, self.nslots = len(jobs), int(nslots)
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
        self.out = torch.zeros(self.nslots, 2, dtype=torch.int32, device=self.device)

    def launch(self):
        call('yolo2_absmax', ptr(self.table), self.n, ptr(self.out), _stream())

    def result(self):
        words = self.out.cpu().numpy().view(np.uint32)
        return np.ascontiguousarray(words[:, 0]).view(np.float32).copy(), words[:, 1].astype(np.int64)


CALIB_BINS, CALIB_WORDS = _lib.CALIB_BINS, _lib.CALIB_WORDS


class CalibHistogramJobs(object):
    """Device job table of yolo2_calib_histogram over a fixed list of tensors, with its running records.

    ``jobs``: [(tensor, rows, c, ld, slot, limit)] -- as AbsmaxJobs, plus the range [0, limit] of the record's CALIB_BINS bins (finite, > 0;
    jobs that share a slot carry the same limit).  ``launch()`` adds the tensors' current contents to the records (``out``: int64
    [nslots, CALIB_WORDS] on the device, holding the kernel's u64 words); ``result()`` -> (histograms int64 [nslots, CALIB_BINS], non-finite
    counts int64 [nslots], counts of values above the limit int64 [nslots])."""

    def __init__(self, jobs, nslots, device=None):
        from ._lib import CalibJob
        assert len(jobs) > 0
        self.tensors = [j[0] for j in jobs]
        self.device = device if device is not None else self.tensors[0].device
        arr = (CalibJob * len(jobs))()
        self.limits = {}
        for d, (t, rows, c, ld, slot, limit) in zip(arr, jobs):
            rows, c, ld, slot, limit = int(rows), int(c), int(ld), int(slot), np.float32(limit)
            assert t.is_cuda and t.is_contiguous() and 0 < c <= ld and rows > 0 and 0 <= slot < nslots, (rows, c, ld, slot)
            assert (rows - 1) * ld + c <= t.numel(), 'histogram job of %d elements on a tensor of %d' % ((rows - 1) * ld + c, t.numel())
            assert rows * ld <= 2 ** 40, (rows, ld)
            assert np.isfinite(limit) and limit > 0, 'histogram limit %r' % (limit,)
            with np.errstate(all='ignore'):
                inv_width = np.float32(CALIB_BINS) / limit             # f32: the kernel's one multiply uses exactly this value
            assert np.isfinite(inv_width), 'histogram limit %r is too small' % (limit,)
            assert self.limits.setdefault(slot, limit) == limit, 'the jobs of slot %d disagree on the limit' % slot
            d.base, d.rows, d.c, d.ld, d.dtype, d.slot, d.limit, d.inv_width = t.data_ptr(), rows, c, ld, dtype_code(t.dtype), slot, limit, inv_width
        self.n, self.nslots = len(jobs), int(nslots)
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
        self.out = torch.zeros(self.nslots, CALIB_WORDS, dtype=torch.int64, device=self.device)

    def launch(self):
        call('yolo2_calib_histogram', ptr(self.table), self.n, ptr(self.out), _stream())

    def result(self):
        words = self.out.cpu().numpy().view(np.uint64)
        assert int(words.max()) < 2 ** 63
        words = words.astype(np.int64)
        return words[:, :CALIB_BINS].copy(), words[:, CALIB_BINS].copy(), words[:, CALIB_BINS + 1].copy()


def quantize(X, ldx, Q, ldq, rows, c, inv_s):
    call('yolo2_quantize', ptr(X), ldx, ptr(Q), ldq, rows, c, float(inv_s), dtype_code(X.dtype), _stream())


def maxpool_i8(A, lda, P, ldp, B, H, W, C, stride):
    call('yolo2_maxpool_i8', ptr(A), lda, ptr(P), ldp, B, H, W, C, stride, _stream())


def reorg_i8(x, out, B, H, W, C, ldo):
    call('yolo2_reorg_i8', ptr(x), ptr(out), B, H, W, C, ldo, _stream())
