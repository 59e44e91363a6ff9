"""Training / detection sessions: the counterpart of what the reference's callers drive through
``slim.learning.train`` (train.py:109-145) and ``sess.run`` (detect.py:69-71)."""
import math
import os

import numpy as np
import torch

from . import distill as _distill
from . import ops, options
from .engine import Engine, layer_end_offsets, staggered
from .graph import pad8
from .model.yolo2 import OBJECTIVE_KEYS
from .optim import Optimizer, learning_rate_fn
from .parallel import GradReducer


def _label_shapes(B, cells, C):
    return [(B, cells), (B, cells, C), (B, cells, 4), (B, cells, 2), (B, cells, 2), (B, cells)]


def ema_decay_option(ema_decay, config):
    """The ``ema_decay`` of a TrainSession as a float: the argument, or ``[mi355x] ema_decay`` of the config when the argument is None; absent or 0 = off
    (returned as 0.0).  Anything outside [0, 1) raises ValueError.  Pure host logic."""
    ema_decay = options.read(config, 'ema_decay', ema_decay)
    decay = float(ema_decay)
    if not 0.0 <= decay < 1.0:
        raise ValueError('ema_decay = %r: the decay of the weight average lies in [0, 1) (0 or absent: off)' % (ema_decay,))
    return decay


BOX_LOSSES = options.KEYS['box_loss'].choices


def box_loss_option(box_loss, config):
    """The ``box_loss`` of a TrainSession: the argument, or ``[mi355x] box_loss`` of the config when the argument is None; absent = 'mse'.
    Anything but mse, iou, giou, diou, ciou raises ValueError.  Pure host logic."""
    box_loss = options.read(config, 'box_loss', box_loss)
    name = str(box_loss).strip().lower()
    if name not in BOX_LOSSES:
        raise ValueError('box_loss = %r: the box regression loss is one of %s (absent: mse)' % (box_loss, ', '.join(BOX_LOSSES)))
    return name


CLASS_LOSSES = options.KEYS['class_loss'].choices
LOSS_OPTION_DEFAULTS = {k: options.KEYS[k].default for k in ('box_loss', 'class_loss', 'ignore_thresh', 'rescore', 'label_smoothing', 'focal_gamma')}


def loss_options(config, box_loss=None, class_loss=None, ignore_thresh=None, rescore=None, label_smoothing=None, focal_gamma=None):
    """Every option of the YOLOv2 loss of a TrainSession (DESIGN.md sections 21, 22) as the keyword arguments of ``ops.loss``: each argument, or
    the ``[mi355x]`` key of the same name where the argument is None; absent = off (LOSS_OPTION_DEFAULTS).  An unknown name or a value out of
    range raises ValueError naming the option.  Pure host logic."""
    def number(name, given):
        v = options.read(config, name, given, invalid='not a valid value')
        try:
            return float(v)
        except (TypeError, ValueError):
            raise ValueError('%s = %r: a number' % (name, v))
    out = {'box_loss': box_loss_option(box_loss, config)}
    cls = options.read(config, 'class_loss', class_loss)
    out['class_loss'] = str(cls).strip().lower()
    if out['class_loss'] not in CLASS_LOSSES:
        raise ValueError('class_loss = %r: the class term is one of %s (absent: mse)' % (cls, ', '.join(CLASS_LOSSES)))
    t = number('ignore_thresh', ignore_thresh)
    if not (t == 0.0 or 0.0 < t < 1.0):
        raise ValueError('ignore_thresh = %r: the ignore threshold lies inside (0, 1) (0 or absent: off)' % (t,))
    r = options.read(config, 'rescore', rescore, invalid='not a valid value')
    if r not in (False, True, 0, 1):
        raise ValueError('rescore = %r: true or false' % (r,))
    eps = number('label_smoothing', label_smoothing)
    if not 0.0 <= eps < 1.0:
        raise ValueError('label_smoothing = %r: lies in [0, 1) (0 or absent: off)' % (eps,))
    if eps != 0.0 and out['class_loss'] == 'mse':
        raise ValueError('label_smoothing = %r with class_loss = mse: smoothing belongs to the ce and focal class terms' % (eps,))
    gamma = number('focal_gamma', focal_gamma)
    if out['class_loss'] == 'focal' and not (gamma == 0.0 or 1.0 <= gamma < float('inf')):       # (read with focal only, as ops.loss_options and the library do)
        raise ValueError('focal_gamma = %r: 0 or at least 1 (absent: 2)' % (gamma,))
    out.update(ignore_thresh=t, rescore=bool(r), label_smoothing=eps, focal_gamma=gamma)
    return out


def loss_options_set(resolved):
    """The names of the options of ``loss_options`` that are on, box_loss aside (focal_gamma counts only with the focal class term)."""
    return [k for k in ('class_loss', 'ignore_thresh', 'rescore', 'label_smoothing') if resolved[k] != LOSS_OPTION_DEFAULTS[k]]


WEIGHT_DECAY_MODES = options.KEYS['weight_decay_mode'].choices


def recipe_options(config, accum_steps=None, weight_decay=None, weight_decay_mode=None):
    """``accum_steps``, ``weight_decay`` and ``weight_decay_mode`` of a TrainSession as (int, float, str): each argument, or the
    ``[mi355x]`` key of the same name where the argument is None; absent = (1, 0.0, 'l2'), which is off.  A value out of range raises ValueError naming
    the key.  Pure host logic."""
    k = options.read(config, 'accum_steps', accum_steps, how='text')           # (the texts: the refusals quote them)
    try:
        steps = int(str(k).strip())
    except ValueError:
        steps = 0
    if steps < 1:
        raise ValueError('accum_steps = %r: the micro-batches of one update, an integer >= 1 (1 or absent: off)' % (k,))
    d = options.read(config, 'weight_decay', weight_decay, how='text')
    try:
        decay = float(d)
    except (TypeError, ValueError):
        decay = -1.0
    if not 0.0 <= decay < float('inf'):
        raise ValueError('weight_decay = %r: a number >= 0 (0 or absent: off)' % (d,))
    mode = str(options.read(config, 'weight_decay_mode', weight_decay_mode)).strip().lower()
    if mode not in WEIGHT_DECAY_MODES:
        raise ValueError('weight_decay_mode = %r: one of %s (absent: l2)' % (mode, ', '.join(WEIGHT_DECAY_MODES)))
    return steps, decay, mode


def refuse_recipe(accum_steps, weight_decay, weight_decay_mode, v1, shard_optimizer, optimizer):
    """What gradient accumulation and weight decay do not cover, each refusal naming its key; called before anything touches the device."""
    if accum_steps > 1 and v1:
        raise NotImplementedError('accum_steps = %d covers the YOLOv2 family: the dropout masks of YOLO (v1) are drawn per global_step, every micro-batch of '
                                  'an update would get the same one' % accum_steps)
    on = ['accum_steps = %d' % accum_steps] * (accum_steps > 1) + ['weight_decay = %g' % weight_decay] * (weight_decay > 0)
    if on and shard_optimizer:
        raise NotImplementedError('[mi355x] shard_optimizer with %s: the sharded update runs inside the bucket chains during backward, before the '
                                  'accumulated gradient exists; turn one of them off' % on[0])
    if weight_decay > 0 and weight_decay_mode == 'decoupled' and optimizer == 'ftrl':
        raise NotImplementedError('weight_decay_mode = decoupled with the ftrl optimizer: FTRL recomputes a weight from its accumulators, a shrunk weight '
                                  'would be overwritten; use weight_decay_mode = l2 (or [optimizer_ftrl] l2_regularization_strength)')


def decay_ranges(param_offsets):
    """The element ranges of the parameter arena that weight decay covers: the variables named .../weights (convolution and fully connected filters; gamma,
    beta and biases are not decayed -- Darknet's choice), sorted by offset.  Pure host logic."""
    return sorted((o, o + n) for name, (o, n) in param_offsets.items() if name.rsplit('/', 1)[-1] == 'weights')


def ema_decay_at(ema_decay, t):
    """[TF-sem] tf.train.ExponentialMovingAverage(decay, num_updates=t): min(decay, (1 + t) / (10 + t)), in Python floats."""
    return min(ema_decay, (1.0 + t) / (10.0 + t))


class TrainSession(object):
    """One training replica.  ``step`` = per-image standardisation -> forward (batch-stat BN, EMA
    update first: [TF-sem] UPDATE_OPS) -> loss + its gradient -> backward -> (all-reduce) -> optional
    per-tensor clip -> optimizer; all asynchronous on the current stream."""

    def __init__(self, builder, batch_size, dtype='bf16', optimizer='adam', learning_rate=1e-6, gradient_clip=0.0,
                 config=None, seed=0, world_size=1, bucket_mb=64.0, preprocess_mode=0, sizes=None, grad_dtype='f32', comm_cus=None, comm_timing=False,
                 sync_bn=False, shard_optimizer=False, deterministic=None, ema_decay=None, box_loss=None,
                 class_loss=None, ignore_thresh=None, rescore=None, label_smoothing=None, focal_gamma=None,
                 accum_steps=None, weight_decay=None, weight_decay_mode=None, teacher=None, distill=None):
        """``sizes``: optional list of (width, height) input sizes for multi-scale training (BASELINE configs[3]); buffers are
        allocated once for the largest, ``set_size`` switches between them, the builder's configured size is selected first.

        ``deterministic``: bitwise reproducible steps (deterministic training mode) -- same parameters, optimizer slots, BN state,
        global_step, image tensor and labels => bitwise the same state after ``step()``, whatever the buffer addresses, the process or the
        run.  None (default): on when ``[mi355x] deterministic`` of the config is true or YOLO2_DETERMINISTIC=1 is set; False / True decide here.  YOLOv2
        family only; with world_size > 1 the local computation is deterministic but nothing is promised across the collective.

        ``ema_decay``: exponential moving average of the trainable arena (weight averaging), updated once per step after the optimizer.
        None (default): ``[mi355x] ema_decay`` of the config; absent or 0: off -- ``session.ema`` is None, nothing is allocated or launched.

        ``box_loss``: the box regression term of the YOLOv2 loss: 'mse' (the reference's squared error) or 'iou', 'giou',
        'diou', 'ciou'.  None (default): ``[mi355x] box_loss`` of the config; absent or 'mse': the loss call made before the option existed.

        ``class_loss`` ('mse' | 'ce' | 'focal'), ``ignore_thresh``, ``rescore``, ``label_smoothing``, ``focal_gamma``: the other options of the
        YOLOv2 loss.  None (default): the ``[mi355x]`` key of the same name; absent: off, the loss call as it was.

        ``accum_steps`` = K: gradient accumulation (Darknet's subdivisions).  ``step()`` is then one MICRO-batch: K - 1 of them run forward,
        loss and backward and add their gradient into a second arena, the K-th forms the mean and updates; ``micro_step`` counts 0 .. K - 1, ``global_step``
        counts updates.  ``weight_decay`` with ``weight_decay_mode`` 'l2' (wd * w joins the gradient of the filters before the collective, the clip and the
        optimizer) or 'decoupled' (AdamW: the filters are scaled by 1 - lr * wd ahead of the update).  None (default): the ``[mi355x]`` key of the same
        name; absent, 1 and 0: off -- nothing is allocated, no launch is added.

        ``teacher``: a ``DetectSession`` of a YOLOv2 network with this one's anchors, classes and grids, restored by the caller, for objectness-scaled
        distillation: every ``forward_backward`` runs the teacher's forward on the same images and adds the gradient of the weighted
        distill term into the logit gradient, behind the loss.  With ``sizes`` the teacher is built with the same sizes; ``set_size`` switches both.
        ``distill``: a dict of the ``[distill]`` keys weight, objectness, coords, prob, class_term, temperature, scale_by_objectness
        (yolo_tf_amd/distill.py); a key it lacks, or None, is read from the config's section, else its default.  ``teacher`` None or weight 0: off --
        ``session.teacher`` is None, nothing is allocated or launched."""
        assert builder.training, 'call builder(data, training=True) first'
        cfg = config if config is not None else getattr(builder, 'config', None)         # the one config every option below is read from
        self.accum_steps, self.weight_decay, self.weight_decay_mode = recipe_options(cfg, accum_steps, weight_decay, weight_decay_mode)
        refuse_recipe(self.accum_steps, self.weight_decay, self.weight_decay_mode, getattr(builder, 'family', 'yolo2') == 'yolo', shard_optimizer, optimizer)
        self._recipe = self.accum_steps > 1 or self.weight_decay > 0          # False: step() is the step it was before the options existed
        self.micro_step = 0
        self._update_due = False             # True between the last micro-batch's forward_backward() and its apply_gradients()
        self.ema_decay = ema_decay_option(ema_decay, cfg)
        self.loss_options = loss_options(cfg, box_loss, class_loss, ignore_thresh, rescore, label_smoothing, focal_gamma)
        self.box_loss = self.loss_options['box_loss']
        self.builder = builder
        self.B = batch_size
        own = (builder.width, builder.height)
        traced = {own: (builder.graph, builder.model)}
        self.v1 = getattr(builder, 'family', 'yolo2') == 'yolo'       # YOLO (v1): linear fully connected head, boxes_per_cell instead of anchors
        if self.v1 and self.box_loss != 'mse':
            raise NotImplementedError('box_loss = %s covers the YOLOv2 family: the YOLO (v1) loss regresses its boxes with the squared error only' % self.box_loss)
        on = loss_options_set(self.loss_options)
        if self.v1 and on:
            raise NotImplementedError('%s = %s covers the YOLOv2 family: the YOLO (v1) loss has its own objectness and class terms only' % (on[0], self.loss_options[on[0]]))
        assert not (self.v1 and sizes), 'the fully connected YOLO (v1) head fixes the input size'
        for wh in (sizes or []):
            wh = (int(wh[0]), int(wh[1]))
            if wh not in traced:
                traced[wh] = builder.trace(wh[0], wh[1], training=True)
        largest = max(traced, key=lambda wh: wh[0] * wh[1])
        assert all(w <= largest[0] and h <= largest[1] for w, h in traced), 'one size must contain all the others'
        self.teacher, self.distill = None, None
        if teacher is not None:
            resolved = _distill.options(cfg, **(distill or {}))
            if resolved['weight'] > 0:
                _distill.refuse_pair(_distill.head({wh: gm[1] for wh, gm in traced.items()}, self.v1, batch_size),
                                     _distill.head(teacher.models, teacher.v1, teacher.B, int8=getattr(teacher, 'dtype', None) == 'int8'))
                self.teacher, self.distill = teacher, _distill.kernel_options(resolved)
        if deterministic is None:
            deterministic = options.read(cfg, 'deterministic') or os.environ.get('YOLO2_DETERMINISTIC', '0') == '1'
        self.deterministic = bool(deterministic)
        if self.deterministic and self.v1:
            raise NotImplementedError('deterministic=True covers the YOLOv2 family: the YOLO (v1) loss and fully connected head still sum in arrival order')
        if self.deterministic and world_size > 1:
            import logging
            logging.getLogger(__name__).warning('deterministic=True with world_size = %d: each replica computes its gradients in a fixed order, '
                                                'but no bitwise promise is made across the gradient collective', world_size)
        self.engine = Engine(traced[largest][0], batch_size, dtype, training=True, seed=seed, sync_bn=sync_bn and world_size > 1,
                             side_priority=-1 if world_size == 1 else 0, deterministic=self.deterministic)
        e = self.engine
        if e.sync_bn:                # batch moments and BN-backward sums over all replicas ([mi355x] sync_bn; default: replica-local like N reference processes)
            import torch.distributed as dist
            # a group of its own: a process group's collectives run in order on one internal stream, so the small per-layer BN exchanges
            # would otherwise queue behind whatever 64 MB gradient bucket is on the wire (every rank builds its session: new_group is collective)
            e.bn_group, e.bn_world = (dist.new_group() if dist.is_initialized() else dist.group.WORLD), int(world_size)
        self.models = {wh: gm[1] for wh, gm in traced.items()}
        m0 = traced[largest][1]
        self.A, self.C = (m0.boxes_per_cell if self.v1 else len(m0.anchors)), m0.classes
        dev = e.device
        self.anchors = None if self.v1 else torch.from_numpy(m0.anchors.reshape(-1)).to(dev)
        self._labels = {wh: [torch.zeros(*s, dtype=torch.float32, device=dev) for s in _label_shapes(batch_size, mdl.cells, self.C)]
                        for wh, mdl in self.models.items()}
        self.objectives_dev = torch.zeros(4, dtype=torch.float32, device=dev)
        self.loss_ws = torch.zeros(ops.loss_ws_floats(batch_size, m0.cells, self.A), dtype=torch.float32, device=dev)
        for wh, (g, _) in traced.items():
            if wh != largest:
                e.add_size(g)
        if self.teacher is not None:
            # three partial sums per workgroup and the three reduced terms; a teacher session that holds more images than this one reads them from a
            # buffer of its own size whose first B images are the batch (its moving-average BN keeps the images independent)
            self.distill_ws = torch.zeros(ops.distill_ws_floats(batch_size, m0.cells, self.A), dtype=torch.float32, device=dev)
            self.distill_dev = torch.zeros(3, dtype=torch.float32, device=dev)
            self._teacher_images = torch.zeros(self.teacher.B * largest[0] * largest[1] * 3, dtype=torch.float32, device=dev) if self.teacher.B > batch_size else None
            self._distill_pending = None
        self.size = None
        self.set_size(*own)
        self.hparam = [builder.hparam[k] for k in OBJECTIVE_KEYS]
        self.optimizer = Optimizer(optimizer, cfg, e.n_params, dev)
        self.lr_fn = learning_rate_fn(cfg, learning_rate)
        self.gradient_clip = float(gradient_clip)
        self.clip_ws = torch.zeros(ops.workspace_bytes('clip_fixed' if self.deterministic else 'clip', e.n_seg) // 8, dtype=torch.float64, device=dev)
        self.global_step = 0
        self.world_size = world_size
        self.preprocess_mode = preprocess_mode
        # [mi355x] shard_optimizer: reduce-scatter / update 1/world / all-gather instead of all-reduce + the replicated optimizer pass
        # (parallel.GradReducer); per-tensor clipping needs every complete gradient first, so it keeps the replicated form
        self.shard_optimizer = bool(shard_optimizer) and world_size > 1 and self.gradient_clip <= 0
        if shard_optimizer and world_size > 1 and not self.shard_optimizer:
            import logging
            logging.getLogger(__name__).warning('[mi355x] shard_optimizer is ignored: gradient_clip = %g needs every complete gradient, the update stays replicated',
                                                self.gradient_clip)
        # False between a sharded update and gather_optimizer_state(): this rank's optimizer slots then hold other ranks' shards from an
        # earlier gather (or their initial values) -- checkpoint.save / tf_checkpoint.save refuse to write them
        self.optimizer_state_complete = True
        self.reducer = GradReducer(e.grads, list(e.param_offsets.values()), bucket_mb, grad_dtype=grad_dtype, timing=comm_timing,
                                   shard_params=e.params if self.shard_optimizer else None) if world_size > 1 else None
        if world_size > 1:
            # the collectives' persistent kernels hold CUs for their whole duration: stream-K launches (one workgroup per CU) are sized
            # for what is left ([mi355x] comm_cus, default 32 -- an RCCL ring's channel count on this part)
            reserve = options.read(cfg, 'comm_cus', comm_cus)
            total = torch.cuda.get_device_properties(dev).multi_processor_count
            ops.set_stream_workgroups(max(64, total - int(reserve)) if reserve > 0 else 0)
        if world_size > 1 and torch.distributed.is_available() and torch.distributed.is_initialized():
            e.dropout_rank = torch.distributed.get_rank()
        self.bucketed_update = True
        self.fuse_adam_prep = os.environ.get('YOLO2_FUSE_ADAM_PREP', '1') != '0'      # A/B: 0 = Adam launch + separate operand re-layout at the next forward
        # Candidate, OFF by default (YOLO2_EARLY_ADAM=1 enables it): single process, Adam, no clipping -- a layer's filter is updated as soon as
        # its gradient is final, on a third stream, while backward goes on (the update is HBM-bound, 0.36-0.41 ms as one launch at the end of the
        # step; the 13x13 layers whose gradients come first hold 84 % of the parameters).  Bit-identical to the one-launch form (same kernel per
        # layer, tests/test_network_gpu.py).  Measured SLOWER: 3.72 vs 3.62 ms per step (profiles/r05_early_adam.txt) -- the update's thousands
        # of small workgroups (16.6 KB of LDS each) occupy CUs that the 150 KB convolution workgroups then cannot be placed on.
        self.early_adam = (os.environ.get('YOLO2_EARLY_ADAM', '0') == '1' and not self.deterministic and world_size == 1 and optimizer == 'adam' and self.fuse_adam_prep
                           and self.gradient_clip <= 0 and not getattr(e, '_has_l2', False) and dev.type == 'cuda' and not self._recipe)
        self.opt_stream = torch.cuda.Stream(device=dev) if self.early_adam else None
        self._early_pending = False
        self._in_step = False            # the early-update candidate only runs inside step(): forward_backward() + apply_gradients() as one unit
        # device-detected failures (a stream-K tile owner that gave up, conv_shared.h) polled every step without a synchronisation
        self.async_errors = ops.AsyncErrorPoll() if dev.type == 'cuda' else None
        # arena offset below which every gradient is final once a given layer's backward has run
        self._layer_end = layer_end_offsets(e.graph, e.param_offsets)
        # [TF-sem] tf.train.ExponentialMovingAverage: one shadow per trainable variable, at the variable's own range of an arena laid out like
        # engine.params, starting at the variable's initial value (no zero-debias).  The BN moving statistics (engine.state) are averages already.
        self.ema, self.ema_var = None, {}
        if self.ema_decay > 0:
            self.ema = staggered(e.n_params, torch.float32, dev)
            self.ema.copy_(e.params)
            self.ema_var = {name: self.ema[o:o + n] for name, (o, n) in e.param_offsets.items()}
        # gradient accumulation: the running sum of the micro-gradients, an arena laid out like engine.grads (never zeroed: the first micro-batch stores);
        # weight decay: the device table of the filters' ranges (csrc/grad_combine.hip), built once
        self.grad_acc = staggered(e.n_params, torch.float32, dev) if self.accum_steps > 1 else None
        self.decay_table = ops.grad_ranges(decay_ranges(e.param_offsets), e.n_params, dev) if self.weight_decay > 0 else None

    def set_size(self, width, height):
        """Input size of the following steps (one of the sizes the session was built with); weights, statistics, optimizer state
        and global_step carry over.  Labels must be uploaded for the new grid."""
        wh = (int(width), int(height))
        self.engine.set_size(wh[1], wh[0])
        self.model = self.models[wh]
        self.labels = self._labels[wh]
        self.size = wh
        if self.teacher is not None:
            self.teacher.set_size(*wh)

    def upload_labels(self, labels):
        for dst, src in zip(self.labels, labels):
            dst.copy_(torch.from_numpy(np.ascontiguousarray(src, np.float32).reshape(dst.shape)), non_blocking=True)

    def forward_backward(self, images, defer_collectives=False):
        """Gradients are final (all-reduced) on return unless ``defer_collectives``: then the buckets may still be on the wire
        and ``apply_gradients`` consumes them one by one (what ``step`` does).  With ``accum_steps`` > 1 this is micro-batch ``micro_step``: all but the last
        of an update leave their gradient in ``grad_acc`` and advance ``micro_step``; ``apply_gradients`` follows the last one only (``_backward_recipe``)."""
        e, m = self.engine, self.model
        assert not self._early_pending, 'a layer-wise early update is half applied: apply_gradients() must follow the forward_backward() of step()'
        e.dropout_step = self.global_step
        e.zero_grads()
        e.set_images(images, self.preprocess_mode)
        e.forward()
        out = e.output()
        logits, ld = e.act[out]
        dlogits, _ = e.gact[out]
        if self.v1:
            ops.yolo1_loss(logits, ld, self.labels, self.hparam, self.objectives_dev, dlogits, self.loss_ws, self.B, m.cell_height, m.cell_width, self.A, self.C)
        else:
            # (the four objective values are reduced from the partial sums when fetch() asks for them)
            # (box_loss 'mse' is yolo2_loss_partials, the call made before the option existed; the other modes take yolo2_loss_box_partials,
            # any option of section 22 yolo2_loss_ex_partials)
            ops.loss_partials(logits, ld, self.anchors, self.labels, self.hparam, dlogits, self.loss_ws, self.B, m.cell_height, m.cell_width, self.A, self.C,
                              **self.loss_options)
            self._objectives_pending = (m.cell_height, m.cell_width)
            if self.teacher is not None:
                self._distill(images, logits, ld, dlogits)
        if self._recipe:
            self._backward_recipe(defer_collectives)
        elif self.reducer is not None:
            self.reducer.begin()
            # optimizer sharding only inside step(): a bare forward_backward() promises complete (all-reduced) gradients and no update
            self.reducer.shard = self.shard_optimizer and defer_collectives
            self._sharded_pending = self.reducer.shard
            if self.reducer.shard:
                # the update of a bucket's shard runs inside the bucket's chain on the communication stream, while backward continues
                lr, t, gs = self.lr_fn(self.global_step), self.global_step + 1, 1.0 / self.world_size
                self.reducer.update_fn = lambda lo, hi: self.optimizer.apply(e.params, e.grads, lr, t, gs, lo, hi)
            e.backward(on_layer_done=lambda op, ev: self.reducer.ready_upto(self._layer_end[op['name']], ev))
            # without clipping the optimizer consumes the buckets as they arrive (apply_gradients); clipping needs them all
            self._deferred = defer_collectives and self.gradient_clip <= 0 and self.bucketed_update
            self.reducer.finish(wait=not self._deferred)
        elif self.early_adam and defer_collectives and self._in_step:
            hp = self.optimizer.hp
            t = self.global_step + 1
            alpha = self.lr_fn(self.global_step) * math.sqrt(1.0 - hp['beta2'] ** t) / (1.0 - hp['beta1'] ** t)
            main, opt, m_, v_ = torch.cuda.current_stream(), self.opt_stream, self.optimizer.slots[0], self.optimizer.slots[1]

            def update_layer(op, wgrad_done):
                # behind the layer's data gradient on the main stream (it reads the operand the update rewrites) and its filter gradient
                ev = torch.cuda.Event()
                ev.record(main)
                opt.wait_event(ev)
                if wgrad_done is not None:
                    opt.wait_event(wgrad_done)
                with torch.cuda.stream(opt):
                    e.adam_update_layer(op, m_, v_, alpha, hp['beta1'], hp['beta2'], hp['epsilon'], 1.0)
            e.backward(on_layer_done=update_layer)
            self._early_pending = (alpha, hp['beta1'], hp['beta2'], hp['epsilon'])
        else:
            e.backward()

    def _distill(self, images, logits, ld, dlogits):
        """The teacher's forward on this batch, then the distill launch: d(weighted distill term)/d logits is added into ``dlogits``, which the loss has
        just written, and the partial sums of the three terms stay in ``distill_ws`` until ``fetch`` asks.  Same stream: the launch runs behind both
        forwards and ahead of the backward.  In deterministic mode the teacher's convolutions take the fixed-order routes too."""
        m, t = self.model, self.teacher
        if self._teacher_images is not None:
            staged = self._teacher_images[:t.B * images[0].numel()]
            staged[:images.numel()].copy_(images.reshape(-1))
            images = staged
        with ops.deterministic_launches(self.deterministic):
            t_logits, t_ld = t.logits(images, self.preprocess_mode)
        ops.distill_partials(logits, ld, t_logits, t_ld, dlogits, self.distill_ws, self.B, m.cell_height, m.cell_width, self.A, self.C, **self.distill)
        self._distill_pending = (m.cell_height, m.cell_width)

    def _backward_recipe(self, defer_collectives):
        """Backward of micro-batch ``micro_step`` with gradient accumulation and / or weight decay on.  Micro-batches 0 .. K - 2 are
        local: backward, then one launch that stores (the first) or adds the gradient into ``grad_acc`` -- no collective, clip, optimizer or EMA, no
        change of ``global_step``.  The last one: backward without per-layer hooks, then ONE launch that leaves (sum of the micro-gradients) * f32(1 / K), plus
        wd * w over the filters in l2 mode, in ``engine.grads`` (decoupled mode scales the filters by f32(1 - lr * wd) there instead), and only then the
        collective, every bucket at once: the L2 term must be in before a bucket leaves, so this all-reduce is not overlapped with backward."""
        e, K = self.engine, self.accum_steps
        e.backward()
        self._update_due = self.micro_step == K - 1
        if not self._update_due:
            ops.grad_combine(e.grads, self.grad_acc, None, e.n_params, ops.GRAD_STORE if self.micro_step == 0 else ops.GRAD_ADD)
            self.micro_step += 1
            return
        decay, shrink = 0.0, 1.0
        if self.weight_decay > 0 and self.weight_decay_mode == 'l2':
            decay = self.weight_decay
        elif self.weight_decay > 0:
            shrink = float(np.float32(1.0 - self.lr_fn(self.global_step) * self.weight_decay))
            e._filters_dirty = True          # the masters changed under the prepared layouts (the fused Adam launch rewrites them, every other update path marks them too)
        ops.grad_combine(e.grads, self.grad_acc, e.params, e.n_params, ops.GRAD_FINAL, float(np.float32(1.0 / K)), decay, shrink, self.decay_table)
        if self.reducer is not None:
            self.reducer.begin()
            self.reducer.shard = False
            self._sharded_pending = False
            self._deferred = defer_collectives and self.gradient_clip <= 0 and self.bucketed_update
            self.reducer.finish(wait=not self._deferred)

    def apply_gradients(self):
        e = self.engine
        if self._recipe:
            assert self._update_due, 'micro-batch %d of %d: the update follows the last micro-batch' % (self.micro_step, self.accum_steps)
            self._update_due = False
            self.micro_step = 0
        if self.gradient_clip > 0:
            # [TF-sem] clip happens on the (averaged) gradient: scale first when data-parallel
            if self.world_size > 1:
                ops.scale(e.grads, e.n_params, 1.0 / self.world_size)
            if self.deterministic:      # fixed-order sums of squares (64 stored partials per tensor) instead of f64 atomics
                ops.clip_by_norm_fixed(e.grads, e.seg_off, e.n_seg, self.gradient_clip, self.clip_ws)
            else:
                ops.clip_by_norm(e.grads, e.seg_off, e.n_seg, self.gradient_clip, self.clip_ws)
            gscale = 1.0
        else:
            gscale = 1.0 / self.world_size
        lr = self.lr_fn(self.global_step)
        if self._early_pending:
            # every filter was updated during backward (forward_backward); the small parameters follow once the updates have drained
            alpha, b1, b2, eps = self._early_pending
            self._early_pending = False
            torch.cuda.current_stream().wait_stream(self.opt_stream)
            e.adam_update_small(self.optimizer.slots[0], self.optimizer.slots[1], alpha, b1, b2, eps, 1.0)
            self.global_step += 1
            self._update_ema()
            return
        if self.reducer is not None and getattr(self, '_sharded_pending', False):
            # the buckets' chains (reduce-scatter, shard update, all-gather) were enqueued during backward: wait for the last of them
            self.reducer.finish(wait=True)
            self._deferred = False
            self._sharded_pending = False
            self.optimizer_state_complete = False      # own shards only, until gather_optimizer_state()
            self.global_step += 1
            e._filters_dirty = True
        elif self.reducer is not None and getattr(self, '_deferred', False):
            # data parallel: update bucket k while the all-reduces of buckets k+1.. are still in flight -- only the last
            # (smallest: the early layers) bucket's collective is exposed, and the 1.9 GB optimizer pass hides the rest
            for lo, hi in self.reducer.completed_buckets():
                self.optimizer.apply(e.params, e.grads, lr, self.global_step + 1, gscale, lo, hi)
            self._deferred = False
            self.global_step += 1
            e._filters_dirty = True
        elif self.optimizer.name == 'adam' and self.fuse_adam_prep:
            # Adam + the operand layouts of the updated filters in one launch: the next forward finds its filters prepared
            self.optimizer.apply_fused_with_filter_prep(e, lr, self.global_step + 1, gscale)
            self.global_step += 1
        else:
            self.optimizer.apply(e.params, e.grads, lr, self.global_step + 1, gscale)
            self.global_step += 1
            e._filters_dirty = True
        self._update_ema()

    def _update_ema(self):
        """The step's one launch over the shadow arena, behind the final parameters on the current stream; t = the global step AFTER the update."""
        if self.ema is None:
            return
        decay = ema_decay_at(self.ema_decay, self.global_step)
        ops.ema_update(self.ema, self.engine.params, self.engine.n_params, float(np.float32(1.0 - decay)))

    def reset_ema(self):
        """Shadows := the current parameters (a device copy): a checkpoint without shadows, or a transfer, was restored."""
        if self.ema is not None:
            self.ema.copy_(self.engine.params)

    def gather_optimizer_state(self):
        """With optimizer sharding every rank holds valid optimizer slots for its own shards only: all-gathers them (collective: every rank
        calls it) so that the rank that writes the checkpoint has the complete state.  No-op for the replicated update."""
        if self.reducer is not None and self.shard_optimizer:
            self.reducer.shard = True
            self.reducer.gather_slots(self.optimizer.slots)
        self.optimizer_state_complete = True

    def step(self, images, labels=None):
        """One training step; with ``accum_steps`` = K > 1 one MICRO-batch: ``global_step`` (and with it the learning rate, the EMA and every checkpoint)
        moves on every K-th call, when ``micro_step`` is back at 0."""
        # a failure the device reported during an EARLIER step (completed snapshot): a single process raises here, at most eight steps late instead of one
        # summary interval; data-parallel callers read async_error_pending() / device_error() and agree on it first (train.py) -- a rank
        # that raised alone would leave its peers waiting in the next collective
        if self.async_errors is not None and self.world_size == 1:
            self.async_errors.raise_if_pending()
        if labels is not None:
            self.upload_labels(labels)
        self._in_step = True
        try:
            self.forward_backward(images, defer_collectives=True)
            if self._recipe and not self._update_due:
                return               # micro-batch 0 .. K - 2 of an update: accumulated, nothing else changes
            self.apply_gradients()
        finally:
            self._in_step = False
        if self.async_errors is not None and self.global_step % 8 == 0:      # (a 32-byte device-to-host copy in the stream: polled every step it cost 0.5 % of it)
            self.async_errors.snapshot()

    def async_error_pending(self):
        """True when a completed per-step snapshot shows a device-detected failure (no synchronisation)."""
        return self.async_errors is not None and self.async_errors.pending()

    def device_error(self):
        """Synchronises and RETURNS the device-detected failure (an exception object) or None: data-parallel callers put it through agree()
        and raise on every rank (train.py), single-process callers may simply call fetch()."""
        try:
            ops.check_async_errors()
        except RuntimeError as exc:
            return exc
        return None

    def fetch(self):
        """Synchronises and returns {'total_loss', 'iou_best', 'iou_normal', 'coords', 'prob'} of the last step
        (the five scalars the reference summarises, config.ini:63); with a teacher also 'distill_objectness', 'distill_coords', 'distill_prob' (the
        unweighted terms) and 'distill' (their weighted sum), which then is part of 'total_loss'.  With ``accum_steps`` > 1 these are the objectives of the last MICRO-batch that ran,
        not a mean over the update's micro-batches."""
        if getattr(self, '_objectives_pending', None):
            ops.loss_objectives(self.loss_ws, self.objectives_dev, self.B, self._objectives_pending[0], self._objectives_pending[1], self.A)
            self._objectives_pending = None
        if self.teacher is not None and self._distill_pending:
            ops.distill_objectives(self.distill_ws, self.distill_dev, self.B, self._distill_pending[0], self._distill_pending[1], self.A)
            self._distill_pending = None
        ops.check_async_errors()           # device-detected failures (a stream-K hand-off that gave up) become exceptions here
        vals = self.objectives_dev.cpu().numpy().astype(np.float64)
        out = {k: float(v) for k, v in zip(OBJECTIVE_KEYS, vals)}
        out['regularization'] = float(self.engine.reg_loss.item())        # slim.l2_regularizer terms (YOLO v1 fully connected layers; 0 for yolo2)
        out['total_loss'] = float(sum(v * w for v, w in zip(vals, self.hparam))) + out['regularization']
        self.builder.objectives.update({k: out[k] for k in OBJECTIVE_KEYS})
        if self.teacher is not None:
            d, o = self.distill_dev.cpu().numpy().astype(np.float64), self.distill
            out.update(zip(_distill.SCALARS[:3], (float(v) for v in d)))
            out['distill'] = float(o['weight'] * (o['objectness'] * d[0] + o['coords'] * d[1] + o['prob'] * d[2]))
            out['total_loss'] += out['distill']
        return out


class DetectSession(object):
    """Forward with moving-average BN + decode + batched on-GPU NMS (detect.py:69-80)."""

    def __init__(self, builder, batch_size=1, dtype='bf16', seed=0, calibration=None, sizes=None, tta=None, tta_rows=None):
        """``sizes``: optional list of (width, height) input sizes one set of weights is run at (YOLO9000, table 3); the network is traced at
        each, the buffers are allocated once for the largest, ``set_size`` switches between them and the builder's configured size is
        selected first.  Not with ``dtype='int8'``: a calibration's engine binds one size.

        ``tta``: optional list of views (width, height, flip) for test-time augmentation (``yolo_tf_amd.tta.parse_views``):
        the first is the base view and must be the builder's configured size, unflipped.  It implies ``sizes`` (the views' sizes); with
        ``dtype='int8'`` or YOLO (v1) only flip-only views are accepted.  The pooled and fused buffers, the fusion's workspace, ``tta_rows``
        and ``tta_flags`` are allocated once, here; ``tta_begin`` / ``tta_add`` / ``tta_fuse`` / ``tta_check`` drive them.  None (default):
        ``session.tta`` is None and nothing is allocated or launched.  ``tta_rows``: rows R of the fused buffers per image, default M (the
        views' boxes together).  A fused row is one (box, class), so at an evaluation's low threshold, where a box passes in several classes,
        an image can need up to M * C rows ('evaluation' asks for ``tta.evaluation_rows(M, C)``); too few is reported by ``tta_check``, never silently cut."""
        assert not builder.training
        self.builder = builder
        self.dtype = dtype
        self.v1 = getattr(builder, 'family', 'yolo2') == 'yolo'
        own = (builder.width, builder.height)
        traced = {own: (builder.graph, builder.model)}
        self.tta = None
        if tta:
            from . import tta as _tta
            self.tta = _tta.normalise(tta)
            if self.tta[0][:2] != own:
                raise ValueError('tta: the base view %dx%d is not the configured input size %dx%d' % (self.tta[0][:2] + own))
            if not _tta.flip_only(self.tta):
                if dtype == 'int8':
                    raise ValueError("dtype='int8' with tta sizes: quantised inference binds one input size (QuantEngine); only flip-only views are accepted")
                if self.v1:
                    raise ValueError('tta sizes: the fully connected YOLO (v1) head fixes the input size; only flip-only views are accepted')
                sizes = list(sizes or []) + [wh for wh in _tta.view_sizes(self.tta) if wh != own]
        if sizes:
            if dtype == 'int8':
                raise ValueError("dtype='int8' with sizes: quantised inference binds one input size (QuantEngine); run one session per size")
            if self.v1:
                raise ValueError('sizes: the fully connected YOLO (v1) head fixes the input size')
            for wh in sizes:
                wh = (int(wh[0]), int(wh[1]))
                if wh not in traced:
                    traced[wh] = builder.trace(wh[0], wh[1], training=False)
        largest = max(traced, key=lambda wh: wh[0] * wh[1])
        if not all(w <= largest[0] and h <= largest[1] for w, h in traced):
            raise ValueError('sizes: one size must contain all the others')
        if dtype == 'int8':
            # post-training quantised inference (yolo_tf_amd/quant.py): int8 activations and filters, bf16 logits -- decode, NMS and the
            # evaluators below read those and do not change
            from .quant import Calibration, QuantEngine
            if self.v1:
                raise NotImplementedError("dtype='int8' covers the YOLOv2 family: the YOLO (v1) fully connected head is not quantised")
            if calibration is None:
                raise ValueError("dtype='int8' needs a calibration (quantize.py writes one; yolo_tf_amd.quant.calibrate makes one)")
            if not isinstance(calibration, Calibration):
                calibration = Calibration.load(calibration)
            self.engine = QuantEngine(builder.graph, batch_size, calibration, seed=seed)
        else:
            self.engine = Engine(traced[largest][0], batch_size, dtype, training=False, seed=seed)
        e = self.engine
        dev = e.device
        for wh, (g, _) in traced.items():
            if wh != largest:
                e.add_size(g)
        if len(traced) > 1:
            # the filters are folded with their BN statistics once, for the layers a binding's plan does not fuse with a
            # pool: every size must fuse the same layers (true of sizes that are multiples of the network's stride)
            fused = set(tuple(sorted(t.name for t in bnd['plan'].fused_pool)) for bnd in e._bindings.values())
            if len(fused) != 1:
                raise ValueError('sizes: the network fuses different layers with their pools at these sizes')
        self.models = {wh: gm[1] for wh, gm in traced.items()}
        m = traced[largest][1]
        self.B, self.A, self.C = batch_size, (m.boxes_per_cell if self.v1 else len(m.anchors)), m.classes
        n = m.cells * self.A
        self.anchors = None if self.v1 else torch.from_numpy(m.anchors.reshape(-1)).to(dev)
        # allocated once for the largest N; every size reads and writes contiguous views at the start
        conf = torch.zeros(batch_size * n * self.C, dtype=torch.float32, device=dev)
        xy_min = torch.zeros(batch_size * n * 2, dtype=torch.float32, device=dev)
        xy_max = torch.zeros(batch_size * n * 2, dtype=torch.float32, device=dev)
        order = torch.zeros(batch_size * n, dtype=torch.int32, device=dev)
        self._outputs = {}
        for wh, mdl in self.models.items():
            k = mdl.cells * self.A
            self._outputs[wh] = (k, conf[:batch_size * k * self.C].view(batch_size, k, self.C), xy_min[:batch_size * k * 2].view(batch_size, k, 2),
                                 xy_max[:batch_size * k * 2].view(batch_size, k, 2), order[:batch_size * k].view(batch_size, k))
        self.nan_flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self._attrs_by_size = {}
        self.nms_ws = torch.zeros(max(ops.workspace_bytes('nms', batch_size, o[0], self.C) for o in self._outputs.values()) // 4,
                                  dtype=torch.int32, device=dev)
        self.async_errors = ops.AsyncErrorPoll()
        if self.tta:
            self._tta_allocate(tta_rows)
        self.size = None
        self.set_size(*own)

    def _tta_allocate(self, rows):
        """The buffers of test-time augmentation, once: pooled [B,M,.] (M = the views' boxes together), fused [B,R,.] with R = ``rows`` or M,
        the fusion's workspace for min(M, 1024) clusters per class (a class cannot open more clusters than it has
        candidates, so a larger max_per_class means the same), rows [B] and the flags word."""
        from . import tta as _tta
        dev, B, C = self.engine.device, self.B, self.C
        self._tta_offset, M = [], 0
        for w, h, _ in self.tta:
            self._tta_offset.append(M)
            M += self._outputs[(w, h)][0]
        if M > _tta.M_LIMIT:
            raise ValueError('tta: the views hold %d boxes per image together, the fusion takes at most %d' % (M, _tta.M_LIMIT))
        if rows == 'evaluation':
            rows = _tta.evaluation_rows(M, C)
        self.tta_M, self.tta_R = M, M if rows is None else int(rows)
        if self.tta_R < 1:
            raise ValueError('tta_rows = %r: the fused buffers hold at least one row' % (rows,))
        self._tta_cap = min(M, 1024)
        f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        self.tta_pooled = (f32(B, M, C), f32(B, M, 2), f32(B, M, 2))
        self.tta_fused = (f32(B, self.tta_R, C), f32(B, self.tta_R, 2), f32(B, self.tta_R, 2))
        self.tta_ws = torch.zeros(ops.workspace_bytes('wbf', B, C, self._tta_cap), dtype=torch.uint8, device=dev)
        self.tta_rows = torch.zeros(B, dtype=torch.int32, device=dev)
        self.tta_flags = torch.zeros(1, dtype=torch.int32, device=dev)

    def tta_begin(self):
        """Before the first batch of a run of ``tta_add`` / ``tta_fuse``: zeroes the overflow flags (``tta_check`` reads them)."""
        self.tta_flags.zero_()

    def tta_add(self, images, view, threshold=0.3, threshold_iou=0.4, preprocess_mode=0, nms='hard', sigma=0.5):
        """One view of the batch: ``set_size``, ``run`` (no synchronisation), the view's own NMS in place, and the gather of its boxes into
        the pooled buffers in base-grid cells.  ``images``: device f32 [B,h,w,3] at the view's size, already mirrored if the view is flipped.
        Returns this view's (conf, xy_min, xy_max) after NMS (the session's buffers, in the view's cells)."""
        view = (int(view[0]), int(view[1]), bool(view[2]))
        v = self.tta.index(view)
        self.set_size(view[0], view[1])
        self.run(images, preprocess_mode, check_numerics=False)
        self.nms(threshold, threshold_iou, nms, sigma)
        m, m0 = self.model, self.models[self.tta[0][:2]]
        sx = np.float32(m0.cell_width) / np.float32(m.cell_width)
        sy = np.float32(m0.cell_height) / np.float32(m.cell_height)
        ops.tta_gather(self.conf, self.xy_min, self.xy_max, *self.tta_pooled, self.B, self.N, self.C, self.tta_M, self._tta_offset[v],
                       sx, sy, m0.cell_width, view[2])
        return self.conf, self.xy_min, self.xy_max

    def tta_fuse(self, threshold=0.3, fuse_iou=0.55, max_per_class=256):
        """Weighted Boxes Fusion of what the ``tta_add`` calls pooled (every view once).  Returns device tensors (conf [B,R,C], xy_min, xy_max
        [B,R,2] in base-grid cells, rows [B] int32): rows[b] fused boxes first, +0.0 after them.  The session is back at the base size."""
        cap = min(int(max_per_class), self._tta_cap)
        ops.wbf(*self.tta_pooled, *self.tta_fused, self.tta_rows, self.tta_flags, self.tta_ws, self.B, self.tta_M, self.C, len(self.tta), cap,
                self.tta_R, float(threshold), float(fuse_iou))
        self.set_size(*self.tta[0][:2])
        return self.tta_fused + (self.tta_rows,)

    def tta_check(self):
        """Synchronises, reads the flags the fusions since ``tta_begin`` left and raises RuntimeError naming the cap that overflowed."""
        flags = int(self.tta_flags.item())
        if flags:
            what = []
            if flags & ops.WBF_FLAG_CANDIDATES:
                what.append('more than %d candidates above the threshold in one (image, class): raise the threshold' % ops.WBF_MAX_CANDIDATES)
            if flags & ops.WBF_FLAG_CLUSTERS:
                what.append('more clusters than max_per_class in one (image, class): raise max_per_class (at most 1024) or the threshold')
            if flags & ops.WBF_FLAG_ROWS:
                what.append('more fused boxes than rows in one image')
            raise RuntimeError('tta: the fusion overflowed (flags %d): %s' % (flags, '; '.join(what)))

    def set_size(self, width, height):
        """Input size of the following runs (one of the sizes the session was built with); the variables are shared."""
        wh = (int(width), int(height))
        if wh not in self.models:
            raise KeyError('input size %dx%d is not one of the sizes the session was built with' % wh)
        if len(self.models) > 1:
            self.engine.set_size(wh[1], wh[0])
        self.model = self.models[wh]
        self.N, self.conf, self.xy_min, self.xy_max, self.order = self._outputs[wh]
        self._attrs = self._attrs_by_size.get(wh)
        self._attrs_valid = False
        self.model.bind(self)        # Model.conf / xy_min / xy_max / iou / prob / xy / wh read this session's buffers
        self.size = wh

    def run(self, images, preprocess_mode=0, check_numerics=True):
        """images: device f32 [B,H,W,3].  Returns device tensors conf [B,N,C], xy_min, xy_max [B,N,2]
        (cell units).  Raises FloatingPointError on NaN/Inf like tf.check_numerics (detect.py:70)."""
        e, m = self.engine, self.model
        e.set_images(images, preprocess_mode)
        e.forward()
        logits, ld = e.act[e.output()]
        self._attrs_valid = False
        self.nan_flag.zero_()
        if self.v1:
            ops.yolo1_head_decode(logits, ld, self.conf, self.xy_min, self.xy_max, self.nan_flag, self.B, m.cell_height, m.cell_width, self.A, self.C)
        else:
            ops.head_decode(logits, ld, self.anchors, self.conf, self.xy_min, self.xy_max, self.nan_flag, self.B, m.cell_height,
                            m.cell_width, self.A, self.C)
        if check_numerics:
            bad = int(self.nan_flag.item()) != 0           # (synchronises: the device-side failure check below then costs one small copy)
            ops.check_async_errors()                      # a stream-K hand-off that gave up: these scores are garbage -- raise like check_numerics
            if bad:
                raise FloatingPointError('conf/xy_min/xy_max : Tensor had NaN or Inf values')
        else:
            # benchmark / pipelined callers: no synchronisation here; a failure of an EARLIER run raises now, this run's is polled by the next
            self.async_errors.raise_if_pending()
            self.async_errors.snapshot()
        return self.conf, self.xy_min, self.xy_max

    def logits(self, images, preprocess_mode=0):
        """``set_images`` plus ``forward``, with no decode and no NMS and no synchronisation: the output tensor [B, cells, ld] (the engine's buffer, in
        its dtype) and its ``ld``.  What a TrainSession reads of its teacher."""
        e = self.engine
        e.set_images(images, preprocess_mode)
        e.forward()
        self._attrs_valid = False
        return e.act[e.output()]

    def attrs(self):
        """iou [B,N], prob [B,N,C], xy, wh [B,N,2] of the last run (model/yolo2/__init__.py:36-56), decoded on first use."""
        if self._attrs is None:
            dev = self.engine.device
            self._attrs = {'iou': torch.zeros(self.B, self.N, dtype=torch.float32, device=dev),
                           'prob': torch.zeros(self.B, self.N, self.C, dtype=torch.float32, device=dev),
                           'xy': torch.zeros(self.B, self.N, 2, dtype=torch.float32, device=dev),
                           'wh': torch.zeros(self.B, self.N, 2, dtype=torch.float32, device=dev)}
            self._attrs_by_size[self.size] = self._attrs
            self._attrs_valid = False
        if not getattr(self, '_attrs_valid', False):
            e, m, a = self.engine, self.model, self._attrs
            logits, ld = e.act[e.output()]
            ops.head_decode_attrs(logits, ld, self.anchors, a['iou'], a['prob'], a['xy'], a['wh'], self.B, m.cell_height, m.cell_width, self.A, self.C)
            self._attrs_valid = True
        return self._attrs

    def nms(self, threshold=0.3, threshold_iou=0.4, method='hard', sigma=0.5):
        """In-place batched NMS on the decoded boxes; returns order [B,N].  method 'hard' is the reference's NMS (csrc/nms.hip; the order is
        the reference's list order); 'linear' and 'gaussian' are Soft-NMS (csrc/soft_nms.hip; the order is by final score, best first)."""
        if method == 'hard':
            ops.nms(self.conf, self.xy_min, self.xy_max, self.order, self.nms_ws, self.B, self.N, self.C, float(threshold), float(threshold_iou))
        elif method in ('linear', 'gaussian'):
            ops.soft_nms(self.conf, self.xy_min, self.xy_max, self.order, self.B, self.N, self.C, method, float(threshold), float(threshold_iou), float(sigma))
        else:
            raise ValueError("nms method must be 'hard', 'linear' or 'gaussian', not %r" % (method,))
        return self.order

    def detect(self, images, threshold=0.3, threshold_iou=0.4, preprocess_mode=0, nms='hard', sigma=0.5):
        self.run(images, preprocess_mode, check_numerics=False)
        self.nms(threshold, threshold_iou, nms, sigma)
        return self.conf, self.xy_min, self.xy_max, self.order
