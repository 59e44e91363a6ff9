#!/usr/bin/env python
"""train.py -- YOLO/YOLOv2 training on MI355X with the reference CLI (ruiminshen/yolo-tf train.py:148-167):

    python train.py -c config.ini config/yolo2/darknet-20.ini -b 16 -o adam -lr 1e-4 -s 1000
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train.py -c ... -b 8

Same flags (-c -t -e -p -s -d -b -o -n -g -lr --seed --summary_secs --save_secs --level --master
--task); same logdir/cachedir layout, auto-resume from the latest checkpoint in logdir, `-d` wipes
it, `-t/-e` transfers variables.  One process per GPU; `-b` is the per-GPU batch.  The reference's
TFRecord/JPEG input pipeline is out of the hot-path scope: batches come from
``--data synthetic`` (seeded generator, default) or ``--data file.npz``: either pre-made labels (images uint8
[N,H,W,3] + the six tensors of utils.data.transform_labels) or decoded images with raw boxes (images,
objects_class [total], objects_coord [total,4] pixels, objects_first [N+1]); the latter goes through the on-device
input pipeline (utils/augment.py: crop / resize / colour augmentation per config.ini [data_augmentation_*], labels
built on the GPU) -- the counterpart of the reference's load_image_labels after JPEG decode.  ``--data cache`` reads the
reference's own TFRecord cache (<cachedir>/<profile>.tfrecord for every ``-p`` profile, utils/tfrecord.py) into HBM.
``--mosaic P`` / ``--mixup P`` (``[mi355x] mosaic``, ``mixup``) compose training images of several dataset images on the device (utils/augment.py).
``--multiscale SPEC`` / ``[mi355x] multiscale`` trains at a size drawn from a list every ``--multiscale_every`` steps (yolo_tf_amd/multiscale.py).
``--box_loss MODE`` / ``[mi355x] box_loss`` regresses the responsible anchor's box with 1 - IoU / GIoU / DIoU / CIoU instead of the squared error (YOLOv2 family).
``--ignore_thresh T``, ``--rescore``, ``--class_loss mse|ce|focal``, ``--label_smoothing E``, ``--focal_gamma G`` (and the ``[mi355x]`` keys of the same names) are the other
options of the YOLOv2 loss: Darknet's ignore threshold, the IoU objectness target, a cross-entropy or focal class term.
``--teacher CFG [CFG ...]`` / ``[distill] teacher`` distils the network from a trained YOLOv2 teacher with the same anchors, classes and grid (DESIGN.md section 25;
``--teacher_ckpt``, ``--teacher_ema``, ``--teacher_dtype``, ``--distill_weight`` ... are the section's other keys).  The teacher is not saved with the student: a
resumed run names it again."""
import argparse
import configparser
import logging
import os
import re
import shutil
import time

import numpy as np
import torch

from yolo_tf_amd import checkpoint, multiscale, options, tf_checkpoint, utils
from yolo_tf_amd import distill as distillation
from yolo_tf_amd.utils import events
from yolo_tf_amd.parallel import agree, init_distributed, sync_replicas
from yolo_tf_amd.optim import LR_KEYS, learning_rate_fn
from yolo_tf_amd.session import TrainSession, box_loss_option, loss_options, loss_options_set, recipe_options, refuse_recipe
from yolo_tf_amd.summary import HistogramSummaries, ImageSummaries
from yolo_tf_amd.utils import data as udata


def make_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('-c', '--config', nargs='+', default=['config.ini'], help='config file')
    parser.add_argument('-t', '--transfer', help='transferring model from a checkpoint file')
    parser.add_argument('-e', '--exclude', nargs='+', help='exclude variables while transferring')
    parser.add_argument('-p', '--profile', nargs='+', default=['train', 'val'])
    parser.add_argument('-s', '--steps', type=int, default=None, help='max number of steps')
    parser.add_argument('-d', '--delete', action='store_true', help='delete logdir')
    parser.add_argument('-b', '--batch_size', default=8, type=int, help='batch size (per GPU)')
    parser.add_argument('-o', '--optimizer', default='adam')
    parser.add_argument('-n', '--logname', default=time.strftime('%Y-%m-%d_%H-%M-%S'), help='run name')
    parser.add_argument('-g', '--gradient_clip', default=0, type=float, help='gradient clip')
    parser.add_argument('-lr', '--learning_rate', default=1e-6, type=float, help='learning rate')
    parser.add_argument('--seed', type=int, default=None)
    parser.add_argument('--summary_secs', default=30, type=int, help='seconds between logged summaries')
    parser.add_argument('--save_secs', default=600, type=int, help='seconds to save model')
    parser.add_argument('--level', help='logging level')
    parser.add_argument('--master', default='', help='accepted for compatibility (rendezvous comes from torch.distributed.run)')
    parser.add_argument('--task', type=int, default=0, help='accepted for compatibility (rank comes from RANK)')
    parser.add_argument('--data', default='cache', help="'cache' (default, as the reference's train.py:98-100: the TFRecord cache of the -p profiles under cachedir), "
                        "'synthetic' (random images and labels: benchmarking / smoke runs) or a .npz file")
    parser.add_argument('--dtype', default=None, choices=['bf16', 'f32'], help='overrides [mi355x] dtype')
    parser.add_argument('--deterministic', action='store_true', help='bitwise reproducible training steps (also [mi355x] deterministic / YOLO2_DETERMINISTIC=1): '
                        'filter gradients summed through a workspace in a fixed order, no float atomics anywhere in the step')
    parser.add_argument('--rescore', default=None, action='store_true', help="[mi355x] rescore: the responsible anchor's objectness target is its IoU instead of 1")
    parser.add_argument('--no_rescore', dest='rescore', action='store_false', help='turns [mi355x] rescore off')
    options.add_flags(parser, ('multiscale', 'multiscale_every', 'mosaic', 'mixup', 'box_loss', 'class_loss', 'ignore_thresh', 'label_smoothing', 'focal_gamma', 'accum_steps',
                               'weight_decay', 'weight_decay_mode', 'lr_policy', 'burn_in', 'lr_steps', 'lr_scales'))
    distillation.add_flags(parser)
    parser.add_argument('--ckpt_format', default='npz', choices=['npz', 'tf'], help="checkpoint container: 'npz' (every optimizer) or 'tf' (TensorFlow V2 bundle, as the reference's tf.train.Saver writes)")
    return parser.parse_args(argv)


class SyntheticData(object):
    """``session`` and ``downsampling`` (multi-scale): images and labels are made at the session's current size."""

    def __init__(self, batch, classes, width, height, cell_width, cell_height, seed, session=None, downsampling=None):
        self.args = (batch, classes, cell_width, cell_height)
        self.gen = torch.Generator(device='cuda').manual_seed(seed)
        self.shape = (batch, height, width, 3)
        self.seed = seed
        self.i = 0
        self.session, self.downsampling = session, downsampling

    def next(self):
        if self.session is not None:
            (w, h), (dw, dh) = self.session.size, self.downsampling
            self.shape, self.args = (self.shape[0], h, w, 3), self.args[:2] + (w // dw, h // dh)
        images = torch.rand(*self.shape, device='cuda', generator=self.gen) * 255.0
        labels = udata.synthetic_batch(*self.args, seed=self.seed * 1000003 + self.i)
        self.i += 1
        return images, labels


class NpzData(object):
    def __init__(self, path, batch, seed, rank, world):
        z = np.load(path)
        self.images = z['images']
        self.labels = [z[k] for k in udata.LABEL_KEYS]
        self.batch = batch
        self.rng = np.random.RandomState(seed)
        self.rank, self.world = rank, world

    def next(self):
        idx = self.rng.randint(0, len(self.images), self.batch * self.world)[self.rank::self.world]
        images = torch.from_numpy(self.images[idx].astype(np.float32)).cuda()
        return images, tuple(l[idx] for l in self.labels)


class DeviceAugmentedData(object):
    """Decoded images + raw boxes resident in HBM -> augmented batch and label tensors, all on the device."""

    def __init__(self, z, batch, width, height, classes, cell_width, cell_height, config, seed, rank, world, session, sizes=None, downsampling=None):
        from yolo_tf_amd.utils.augment import DeviceInputPipeline
        if isinstance(z, tuple):          # (images, objects) already decoded, e.g. from the reference's TFRecord cache
            images, objects = z
        else:
            images = list(z['images'])
            first = z['objects_first']
            objects = [(z['objects_class'][first[i]:first[i + 1]], z['objects_coord'][first[i]:first[i + 1]]) for i in range(len(images))]
        self.pipe = DeviceInputPipeline(images, objects, batch, width, height, classes, cell_width, cell_height, config=config,
                                        seed=seed, rank=rank, world=world, sizes=sizes, downsampling=downsampling)
        self.session = session

    def next(self):
        return self.pipe.next(self.session), None          # labels were written into the session's buffers in place


def multiscale_setting(args, config):
    """[mi355x] multiscale / multiscale_every with the command line's overrides: None (absent or empty: nothing about the run changes) or
    (sizes, every, added) of multiscale.configure.  Raises ValueError for what cannot train at several sizes, before anything is built."""
    setting = multiscale.configure(config, args.multiscale, args.multiscale_every)
    if setting is not None and args.data not in ('synthetic', 'cache') and 'objects_coord' not in np.load(args.data, allow_pickle=True).files:
        raise ValueError('[mi355x] multiscale = %r: --data %s holds ready-made label tensors, which are laid out for one grid; multi-scale training '
                         'needs raw objects (objects_class, objects_coord, objects_first), the dataset cache or synthetic data'
                         % (multiscale.describe(setting[0]), args.data))
    return setting


def compose_setting(args, config):
    """[mi355x] mosaic / mixup and their companions with the command line's overrides (written into ``config``, where the input pipeline reads
    them): None when both are off (nothing about the run changes), otherwise the options of utils.augment.compose_options.  Raises ValueError for
    an invalid key and for data without raw objects, before anything is built."""
    from yolo_tf_amd.utils.augment import compose_options
    options.write(config, args, ('mosaic', 'mixup'))
    composing = compose_options(config)
    if not (composing['mosaic'] > 0 or composing['mixup'] > 0):
        return None
    if args.data == 'synthetic' or (args.data != 'cache' and 'objects_coord' not in np.load(args.data, allow_pickle=True).files):
        raise ValueError('[mi355x] mosaic = %g, mixup = %g: --data %s holds no raw objects; mosaic and MixUp compose training images from decoded '
                         'images and their boxes (objects_class, objects_coord, objects_first in a .npz, or the dataset cache)'
                         % (composing['mosaic'], composing['mixup'], args.data))
    return composing


def box_loss_setting(args, config):
    """[mi355x] box_loss with the command line's override: one of session.BOX_LOSSES.  Raises ValueError for an unknown value and for the YOLO
    (v1) family with anything but mse, before anything is built."""
    box_loss = box_loss_option(args.box_loss, config)
    if box_loss != 'mse' and config.get('config', 'model') == 'yolo':
        raise ValueError('[mi355x] box_loss = %s: the IoU-family box losses cover the YOLOv2 family; the YOLO (v1) loss regresses its boxes with the '
                         'squared error only' % box_loss)
    return box_loss


def loss_setting(args, config):
    """Every loss option ([mi355x] box_loss, class_loss, ignore_thresh, rescore, label_smoothing, focal_gamma) with the command line's overrides, as
    session.loss_options returns them.  Raises ValueError for an invalid value and for the YOLO (v1) family with any option on, before anything is built."""
    box_loss = box_loss_setting(args, config)       # (first: its refusals come before those of the other options)
    resolved = loss_options(config, box_loss, args.class_loss, args.ignore_thresh, args.rescore, args.label_smoothing, args.focal_gamma)
    on = loss_options_set(resolved)
    if on and config.get('config', 'model') == 'yolo':
        raise ValueError('[mi355x] %s = %s: the loss options cover the YOLOv2 family; the YOLO (v1) loss has its own objectness and class terms only' % (on[0], resolved[on[0]]))
    return resolved


def recipe_setting(args, config):
    """[mi355x] accum_steps, weight_decay, weight_decay_mode and the learning-rate schedule's keys with the command line's overrides (written into ``config``,
    where the session and optim.learning_rate_fn read them; -s stands in for an absent lr_max_steps): (accum_steps, weight_decay, weight_decay_mode).
    Raises ValueError / NotImplementedError naming the key for an invalid value or a combination the session refuses, before anything is built."""
    options.write(config, args, ('accum_steps', 'weight_decay', 'weight_decay_mode', 'lr_policy', 'burn_in', 'lr_steps', 'lr_scales'))
    if (options.read(config, 'lr_policy') or '').strip().lower() in ('poly', 'cosine') and not options.has(config, 'lr_max_steps'):
        options.write(config, argparse.Namespace(lr_max_steps=args.steps), ('lr_max_steps',))
    learning_rate_fn(config, args.learning_rate)          # (for its refusals: the schedule has no value to hand on, the session makes its function of the same config)
    recipe = recipe_options(config)
    refuse_recipe(*recipe, v1=config.get('config', 'model') == 'yolo', shard_optimizer=options.read(config, 'shard_optimizer'), optimizer=args.optimizer)
    return recipe


def distill_setting(args, config):
    """The [distill] section with the command line's overrides (yolo_tf_amd/distill.py): None when no teacher is named or the weight is 0 (nothing about
    the run changes), otherwise every key resolved.  Raises ValueError naming the key for an invalid value and for the YOLO (v1) family, before anything is built."""
    resolved = distillation.options(config, **distillation.from_args(args))
    if not distillation.enabled(resolved):
        return None
    if config.get('config', 'model') == 'yolo':
        raise ValueError('[distill] teacher = %s: distillation covers the YOLOv2 family; the YOLO (v1) head has no anchors to pair with a teacher\'s'
                         % ' '.join(resolved['teacher']))
    return resolved


def build_teacher(resolved, width, height, batch_size, sizes):
    """The teacher of a distilling run: a DetectSession of the network the [distill] teacher config files describe, at the student's input size(s) and
    batch, with the weights of [distill] teacher_ckpt or of the latest checkpoint in the teacher's logdir (the .npz container first, else a
    TensorFlow prefix, as detect.py looks for them).  A teacher without a checkpoint is an error: an untrained teacher teaches noise."""
    from yolo_tf_amd.session import DetectSession
    tconfig = configparser.ConfigParser()
    utils.load_config(tconfig, resolved['teacher'])
    model = tconfig.get('config', 'model')
    if model == 'yolo':
        raise ValueError('[distill] teacher = %s: distillation covers the YOLOv2 family; the teacher is a YOLO (v1) network' % ' '.join(resolved['teacher']))
    tconfig.set(model, 'width', str(width))          # the teacher reads the student's images
    tconfig.set(model, 'height', str(height))
    utils.ensure_names(tconfig)
    builder = __import__('yolo_tf_amd.model.' + model, fromlist=['Builder']).Builder(None, tconfig)
    builder(None)
    teacher = DetectSession(builder, batch_size, dtype=resolved['teacher_dtype'], sizes=sizes)
    logdir = utils.get_logdir(tconfig)
    path = os.path.expanduser(os.path.expandvars(resolved['teacher_ckpt']))
    if path:
        if not (os.path.exists(path) or os.path.exists(path + '.index')):
            raise FileNotFoundError('distillation needs a trained teacher: the teacher checkpoint %s does not exist' % path)
        tf_prefix = os.path.exists(path + '.index')
    else:
        path = checkpoint.latest_checkpoint(logdir)
        tf_prefix = path is None
        if tf_prefix:
            path = tf_checkpoint.latest_checkpoint(logdir)
        if path is None:
            raise FileNotFoundError('distillation needs a trained teacher: no teacher checkpoint in %s (train the teacher first, or name its checkpoint '
                                    'with --teacher_ckpt / [distill] teacher_ckpt)' % logdir)
    step = (tf_checkpoint if tf_prefix else checkpoint).restore(path, engine=teacher.engine, ema=resolved['teacher_ema'])
    logging.warning('distillation: teacher %s (%s) from %s (global_step=%d%s)' % (
        tconfig.get(model, 'inference'), resolved['teacher_dtype'], path, step, ', averaged weights' if resolved['teacher_ema'] else ''))
    return teacher


def describe_loss_options(resolved):
    """One line for the log: the options of DESIGN.md section 22 that are on, or None."""
    on = loss_options_set(resolved)
    if not on:
        return None
    parts = ['%s=%s' % (k, resolved[k]) for k in on]
    if resolved['class_loss'] == 'focal':
        parts.append('focal_gamma=%g' % resolved['focal_gamma'])
    return 'loss options: ' + ', '.join(parts)


def main():
    setting = multiscale_setting(args, config)       # (a refusal comes before the process group and the device are touched)
    composing = compose_setting(args, config)
    loss = loss_setting(args, config)
    accum_steps, weight_decay, weight_decay_mode = recipe_setting(args, config)
    distilling = distill_setting(args, config)
    rank, local_rank, world = init_distributed()
    torch.cuda.set_device(local_rank)
    model = config.get('config', 'model')
    logdir = utils.get_logdir(config)
    if args.delete and rank == 0:
        logging.warning('delete logging directory: ' + logdir)
        shutil.rmtree(logdir, ignore_errors=True)
    if world > 1:
        torch.distributed.barrier()          # nobody looks for checkpoints while rank 0 is still deleting them
    utils.ensure_names(config)
    width = config.getint(model, 'width')
    height = config.getint(model, 'height')
    cell_width, cell_height = utils.calc_cell_width_height(config, width, height)
    logging.warning('(width, height)=(%d, %d), (cell_width, cell_height)=(%d, %d)' % (width, height, cell_width, cell_height))
    yolo = __import__('yolo_tf_amd.model.' + model, fromlist=['Builder'])
    builder = yolo.Builder(args, config)
    builder(None, training=True)
    builder.create_objectives()
    dtype = options.read(config, 'dtype', args.dtype or None)
    seed = args.seed if args.seed is not None else 0
    sizes, schedule, downsampling = None, None, None
    if setting is not None:
        sizes, every, added = setting
        downsampling = utils.get_downsampling(config)
        schedule = multiscale.SizeSchedule(sizes, every, seed)
        if added:
            logging.warning('multiscale: the configured size %dx%d was not in the list and is added' % (width, height))
        logging.warning('multiscale: sizes %s, a new draw every %d steps' % (multiscale.describe(sizes), every))
    if composing is not None:
        logging.warning('mosaic: probability %g, scale %g-%g, fill %g; mixup: probability %g, alpha %g' % (
            composing['mosaic'], composing['mosaic_scale'][0], composing['mosaic_scale'][1], composing['mosaic_fill'], composing['mixup'], composing['mixup_alpha']))
    # [distill]: every rank keeps a teacher of its own, restored from the same file; it is not part of the student's checkpoints, a resumed run names it again
    teaching = dict(teacher=build_teacher(distilling, width, height, args.batch_size, sizes), distill=distillation.kernel_options(distilling)) if distilling else {}
    session = TrainSession(builder, args.batch_size, dtype=dtype, optimizer=args.optimizer, learning_rate=args.learning_rate,
                           gradient_clip=args.gradient_clip, config=config, seed=seed, world_size=world, sizes=sizes,
                           **{key: options.read(config, key) for key in ('bucket_mb', 'grad_dtype', 'sync_bn', 'shard_optimizer')},
                           deterministic=True if args.deterministic else None,      # (None: [mi355x] deterministic / YOLO2_DETERMINISTIC decide)
                           accum_steps=accum_steps, weight_decay=weight_decay, weight_decay_mode=weight_decay_mode,
                           **teaching, **loss)          # (always given: --box_loss mse must win over a config key; all off is the call made before the options existed)
    if session.box_loss != 'mse':
        logging.warning('box_loss: %s (1 - %s of the responsible box, weighted by [yolo2_hparam] coords = %g)' % (
            session.box_loss, {'iou': 'IoU', 'giou': 'GIoU', 'diou': 'DIoU', 'ciou': 'CIoU'}[session.box_loss], builder.hparam['coords']))
    if describe_loss_options(session.loss_options):
        logging.warning(describe_loss_options(session.loss_options))
    logging.warning('optimizer=%s, dtype=%s, world=%d, parameters=%d%s' % (args.optimizer, dtype, world, session.engine.n_params,
                                                                          ', ema_decay=%g' % session.ema_decay if session.ema is not None else ''))
    if session.teacher is not None:
        logging.warning('distillation: %s' % ', '.join('%s=%s' % (k, session.distill[k]) for k in distillation.KERNEL_KEYS))
    if accum_steps > 1 or weight_decay > 0:
        logging.warning('accum_steps=%d: effective batch %d (batch %d x accum_steps %d x world %d)%s' % (
            accum_steps, args.batch_size * accum_steps * world, args.batch_size, accum_steps, world,
            ', weight_decay=%g (%s)' % (weight_decay, weight_decay_mode) if weight_decay > 0 else ''))
    # rank 0 alone chooses and reads the checkpoint; the others receive parameters, statistics, optimizer slots and
    # global_step from it (same seed -> same initial weights anyway, but a restore must not depend on what each rank sees)
    # Both containers may sit in one logdir (a run resumed with the other --ckpt_format, or a logdir the reference wrote): the one
    # with the HIGHER global step wins, so a restart never falls back to an older state.  A failure on rank 0 (corrupt file, shape
    # mismatch) is agreed on before anyone enters the broadcast of sync_replicas -- the other ranks would wait there forever.
    error = None
    if rank == 0:
        try:
            latest = checkpoint.latest_checkpoint(logdir)
            latest_tf = tf_checkpoint.latest_checkpoint(logdir)            # a logdir written by the reference (or --ckpt_format tf)
            step_npz = int(re.search(r'model\.ckpt-(\d+)\.npz$', latest).group(1)) if latest else -1
            if latest and step_npz >= tf_checkpoint.checkpoint_step(latest_tf):
                step = checkpoint.restore(latest, session)
                logging.warning('resuming from %s (global_step=%d)' % (latest, step))
            elif latest_tf:
                step = tf_checkpoint.restore(latest_tf, session)
                logging.warning('resuming from TensorFlow checkpoint %s (global_step=%d)' % (latest_tf, step))
            elif args.transfer:
                path = os.path.expanduser(os.path.expandvars(args.transfer))
                logging.warning('transferring from ' + path)
                if os.path.exists(path + '.index'):                     # a TensorFlow checkpoint prefix, like the reference's -t argument
                    tf_checkpoint.restore(path, session, exclude=args.exclude, variables_only=True)
                else:
                    checkpoint.restore(path, session, exclude=args.exclude, variables_only=True)
        except Exception as e:       # noqa: BLE001  (re-raised below, on every rank)
            error = e
    (failed,) = agree([error is not None], session.engine.device)
    if failed:
        raise error if error is not None else RuntimeError('rank 0 could not restore the checkpoint (see its log)')
    sync_replicas(session)
    logging.warning('global_step=%d, learning_rate=%g' % (session.global_step, session.lr_fn(session.global_step)))
    if args.data == 'synthetic':
        data = SyntheticData(args.batch_size, len(builder.names), width, height, cell_width, cell_height, seed * world + rank + 1,
                             session=session if schedule is not None else None, downsampling=downsampling)
    elif args.data == 'cache':
        # the reference's own dataset cache: <cachedir>/<profile>.tfrecord written by its cache.py (train.py:98-100 there)
        from yolo_tf_amd.utils import tfrecord
        cachedir = utils.get_cachedir(config)
        paths = [os.path.join(cachedir, profile + '.tfrecord') for profile in args.profile]
        logging.warning('loading ' + ', '.join(paths))
        data = DeviceAugmentedData(tfrecord.load_dataset(paths), args.batch_size, width, height, len(builder.names), cell_width, cell_height,
                                   config, seed, rank, world, session, sizes=sizes, downsampling=downsampling)
    elif 'objects_coord' in np.load(args.data, allow_pickle=True).files:
        data = DeviceAugmentedData(np.load(args.data, allow_pickle=True), args.batch_size, width, height, len(builder.names), cell_width, cell_height,
                                   config, seed, rank, world, session, sizes=sizes, downsampling=downsampling)
    else:
        data = NpzData(args.data, args.batch_size, seed, rank, world)
    # the reference's summary_writer (train.py:141-145): scalar events under <logdir>/<logname>
    writer = events.FileWriter(os.path.join(logdir, args.logname)) if rank == 0 else None
    # [summary] histogram / gradients (the reference's summary_histogram and summarize_gradients): rank 0 bins its own replica's tensors on the
    # device after a summarised step; with both keys unset nothing is allocated or launched
    histograms = HistogramSummaries(session, config) if rank == 0 else None
    # [summary] image / image_max (the reference's summary_image): the first image_max images of every matched stored activation, made into
    # bytes on the device in the same place; disabled (a missing key, as in the default config) nothing is allocated or launched
    images_summary = ImageSummaries(session, config) if rank == 0 else None
    save = (lambda: tf_checkpoint.save(logdir, session)) if args.ckpt_format == 'tf' else (lambda: checkpoint.save(logdir, session))
    last_summary = last_save = t_rate = time.time()
    n_rate = 0
    sync_every = 1 if world == 1 else 20     # data parallel: decisions only one rank can make are agreed on every 20 steps
    device = session.engine.device
    scheduled = any(options.has(config, key) for key in LR_KEYS)      # a schedule of DESIGN.md section 23: every update's rate at level info
    while args.steps is None or session.global_step < args.steps:
        multiscale.follow(session, schedule)         # (no schedule: nothing; otherwise the size of this step, logged when it changes)
        images, labels = data.next()
        if scheduled and session.micro_step == 0:
            logging.info('update %d: learning_rate=%r' % (session.global_step, session.lr_fn(session.global_step)))
        session.step(images, labels)
        n_rate += 1
        if session.micro_step != 0:
            continue                 # inside an update (accum_steps > 1): nothing is summarised, agreed on or saved until its last micro-batch has run
        last = args.steps is not None and session.global_step >= args.steps
        if not (last or session.global_step % sync_every == 0):
            continue
        now = time.time()
        # every rank takes the same branches: rank 0's clock decides, any rank's non-finite loss stops all of them
        # (a rank that raised alone would leave the others waiting in the next all-reduce)
        want_summary = rank == 0 and (now - last_summary >= args.summary_secs or last)
        want_save = rank == 0 and now - last_save >= args.save_secs
        want_summary, want_save = agree([want_summary, want_save], device)
        # device-detected failures (a stream-K tile owner that gave up waiting: include/yolo2_hip.h yolo2_check_async_errors).  The per-step
        # snapshot is polled without a synchronisation; before anything is summarised or written the synchronising check runs.  Either way the
        # error goes through agree() like shard_error below: one rank raising alone would leave its peers waiting in the next all-reduce, and
        # a checkpoint must not be written from parameters that garbage gradients have updated.
        dev_error = session.device_error() if (want_summary or want_save or last or session.async_error_pending()) else None
        (bad_device,) = agree([dev_error is not None], device)
        if bad_device:
            raise dev_error if dev_error is not None else RuntimeError('another rank reported a device-side failure (stream-K hand-off gave up)')
        if want_summary:
            if histograms is not None and histograms.enabled:
                histograms.collect()             # asynchronous: binned and copied behind the step, read after fetch() below
            if images_summary is not None and images_summary.enabled:
                images_summary.collect()         # likewise
            s = session.fetch()
            shard_error = None
            if hasattr(data, 'pipe'):
                try:
                    data.pipe.check()    # objects outside the grid / bad class ids / negative extents: the reference raises there
                except Exception as e:   # noqa: BLE001  (a shard-local error: agreed on, then raised by every rank)
                    shard_error = e
            (bad_shard,) = agree([shard_error is not None], device)
            if bad_shard:
                raise shard_error if shard_error is not None else RuntimeError('another rank found invalid objects in its data shard')
            rate = n_rate * args.batch_size * world / (time.time() - t_rate)
            if rank == 0:
                writer.add_training_summary(session.global_step, s)
                if histograms.enabled:
                    histograms.write(writer, session.global_step)
                if images_summary.enabled:
                    images_summary.write(writer, session.global_step)
                writer.flush()
                logging.warning('step %d: total_loss=%.6f iou_best=%.6f iou_normal=%.6f coords=%.6f prob=%.6f (%.1f img/s)'
                                % (session.global_step, s['total_loss'], s['iou_best'], s['iou_normal'], s['coords'], s['prob'], rate))
                if 'distill' in s:
                    logging.warning('step %d: distill=%.6f distill_objectness=%.6f distill_coords=%.6f distill_prob=%.6f'
                                    % (session.global_step, s['distill'], s['distill_objectness'], s['distill_coords'], s['distill_prob']))
            (bad,) = agree([not np.isfinite(s['total_loss'])], device)
            if bad:
                raise FloatingPointError('total_loss is not finite (on at least one rank)')
            last_summary, t_rate, n_rate = now, time.time(), 0
        if want_save:
            session.gather_optimizer_state()     # (optimizer sharding: every rank joins the all-gather of the slot shards; a no-op otherwise)
            if rank == 0:
                logging.warning('saved ' + save())
            last_save = now
    session.gather_optimizer_state()
    if rank == 0:
        logging.warning('saved ' + save())
        writer.close()
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    args = make_args()
    config = configparser.ConfigParser()
    utils.load_config(config, args.config)
    logging.basicConfig(format='%(asctime)s %(message)s')
    if args.level:
        logging.getLogger().setLevel(args.level.upper())
    main()
