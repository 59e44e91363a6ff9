#!/usr/bin/env python
"""detect.py -- YOLOv2 detection on MI355X with the reference CLI (ruiminshen/yolo-tf detect.py:122-131):

    python detect.py image_or_dir -c config.ini config/yolo2/darknet-20.ini -p std -t 0.3 --threshold_iou 0.4

Forward (moving-average BN) + decode + NMS all run on the GPU (the reference's NMS is a Python
triple loop on the host, utils/postprocess.py:39-51).  Restores the latest checkpoint of
utils.get_logdir(config).  Import-safe (`std` / `darknet` preprocessors are reused by camera loops,
reference detect_camera.py:33)."""
import argparse
import configparser
import logging
import os

import numpy as np

from yolo_tf_amd import options, utils

PREPROCESS = {'std': 0, 'darknet': 1}


def std(image):
    from yolo_tf_amd.utils import preprocess
    return preprocess.per_image_standardization(image)


def darknet(image):
    from yolo_tf_amd.utils import preprocess
    return preprocess.darknet(image)


def read_image(path):
    """PIL load honouring the EXIF orientation (reference detect.py:41-56)."""
    from PIL import Image, ImageOps
    return ImageOps.exif_transpose(Image.open(path)).convert('RGB')


def detect(sess, names, path, args):
    """Returns [(class name, confidence, xmin, ymin, xmax, ymax in pixels), ...] for one image."""
    import torch
    model = sess.model
    width, height = sess.builder.width, sess.builder.height
    _image = read_image(path)
    image_width, image_height = _image.size
    resized = np.asarray(_image.resize((width, height)), np.uint8).astype(np.float32)
    conf, xy_min, xy_max = sess.run(torch.from_numpy(resized[None]).cuda(), PREPROCESS[args.preprocess])   # raises on NaN/Inf
    order = sess.nms(args.threshold, args.threshold_iou, args.nms, args.sigma)[0].cpu().numpy()
    conf, xy_min, xy_max = conf[0].cpu().numpy(), xy_min[0].cpu().numpy(), xy_max[0].cpu().numpy()
    scale = np.array([image_width / model.cell_width, image_height / model.cell_height], np.float32)
    results = []
    for i in order:                                   # the reference's box list order (--nms hard) or best final score first (Soft-NMS)
        index = int(np.argmax(conf[i]))
        if conf[i, index] > args.threshold:
            (x0, y0), (x1, y1) = xy_min[i] * scale, xy_max[i] * scale
            results.append((names[index], float(conf[i, index]), float(x0), float(y0), float(x1), float(y1)))
    return results


def detect_tta(sess, names, path, args):
    """detect() with test-time augmentation (--tta): the image is resized with PIL to every view's size as above, mirrored on the host for the
    flipped views, and the views' boxes are fused on the device (Weighted Boxes Fusion).  Best fused score first."""
    import torch
    _image = read_image(path)
    image_width, image_height = _image.size
    sess.tta_begin()
    for w, h, flip in sess.tta:
        resized = np.asarray(_image.resize((w, h)), np.uint8).astype(np.float32)
        if flip:
            resized = np.ascontiguousarray(resized[:, ::-1])
        sess.tta_add(torch.from_numpy(resized[None]).cuda(), (w, h, flip), args.threshold, args.threshold_iou, PREPROCESS[args.preprocess], args.nms, args.sigma)
        if int(sess.nan_flag.item()) != 0:            # (tta_add does not synchronise; here every view is checked as sess.run checks one)
            raise FloatingPointError('conf/xy_min/xy_max : Tensor had NaN or Inf values')
    conf, xy_min, xy_max, rows = sess.tta_fuse(args.threshold, args.tta_iou)
    sess.tta_check()                                   # per image: a cap that overflowed raises here
    from yolo_tf_amd import ops
    ops.check_async_errors()                           # a device-detected failure of any view raises as it does behind sess.run
    n = int(rows[0].item())
    conf, xy_min, xy_max = conf[0, :n].cpu().numpy(), xy_min[0, :n].cpu().numpy(), xy_max[0, :n].cpu().numpy()
    model = sess.model                                 # the base view's: the fused boxes are in its cells
    scale = np.array([image_width / model.cell_width, image_height / model.cell_height], np.float32)
    index = conf.argmax(1) if n else np.zeros(0, np.int64)
    score = conf[np.arange(n), index]
    results = []
    for i in np.argsort(-score, kind='stable'):
        (x0, y0), (x1, y1) = xy_min[i] * scale, xy_max[i] * scale
        results.append((names[index[i]], float(score[i]), float(x0), float(y0), float(x1), float(y1)))
    return results


def draw(path, results, out):
    import matplotlib
    matplotlib.use('Agg')
    import itertools
    import matplotlib.patches as patches
    import matplotlib.pyplot as plt
    fig = plt.figure()
    ax = fig.gca()
    ax.imshow(np.asarray(read_image(path)))
    colors = itertools.cycle(plt.rcParams['axes.prop_cycle'].by_key()['color'])
    for (name, c, x0, y0, x1, y1), color in zip(results, colors):
        ax.add_patch(patches.Rectangle((x0, y0), x1 - x0, y1 - y0, linewidth=min(c * 10, 3), edgecolor=color, facecolor='none'))
        ax.annotate('%s (%.1f%%)' % (name, c * 100), (x0, y0), color=color)
    ax.set_xticks([])
    ax.set_yticks([])
    fig.savefig(out)
    plt.close(fig)


def main():
    from yolo_tf_amd import checkpoint
    from yolo_tf_amd.session import DetectSession
    model = config.get('config', 'model')
    yolo = __import__('yolo_tf_amd.model.' + model, fromlist=['Builder'])
    utils.ensure_names(config)
    builder = yolo.Builder(args, config)
    builder(None)
    dtype = options.read(config, 'dtype', args.dtype or None)
    args.nms, args.sigma = utils.nms_options(args, config)      # --nms / --sigma, else [mi355x] nms / nms_sigma, else hard
    from yolo_tf_amd import tf_checkpoint
    logdir = utils.get_logdir(config)
    calibration = None
    if dtype == 'int8':       # post-training quantised inference: the scales quantize.py measured for this checkpoint
        from yolo_tf_amd import quant
        calibration = quant.calibration_path(logdir, args.calibration)
    # test-time augmentation: --tta / --tta_iou, else [mi355x] tta / tta_iou
    from yolo_tf_amd import tta
    spec, args.tta_iou = tta.options(config, args.tta, args.tta_iou)
    views = tta.parse_views(spec, (builder.width, builder.height), *(utils.get_downsampling(config) if model != 'yolo' else (1, 1)))
    if views:
        logging.info('test-time augmentation: views %s, fused at IoU %g' % (tta.describe(views), args.tta_iou))
        if not tta.flip_only(views):
            from yolo_tf_amd import multiscale
            multiscale.check_nested(tta.view_sizes(views), '--tta %r' % spec)
    sess = DetectSession(builder, 1, dtype=dtype, calibration=calibration, tta=views or None, tta_rows='evaluation' if views else None)
    model_path = checkpoint.latest_checkpoint(logdir)
    tf_path = None if model_path else tf_checkpoint.latest_checkpoint(logdir)      # a logdir the reference trained (tf.train.latest_checkpoint, detect.py:104)
    if model_path is None and tf_path is None:
        raise FileNotFoundError('no checkpoint in ' + logdir)
    logging.info('load ' + (model_path or tf_path))
    step = checkpoint.restore(model_path, engine=sess.engine, ema=args.ema) if model_path else tf_checkpoint.restore(tf_path, engine=sess.engine, ema=args.ema)
    logging.info('global_step=%d' % step)
    path = os.path.expanduser(os.path.expandvars(args.path))
    paths = [path] if os.path.isfile(path) else [os.path.join(d, f) for d, _, fs in os.walk(path) for f in fs
                                                 if os.path.splitext(f)[-1].lower() in args.exts]
    for _path in paths:
        results = (detect_tta if views else detect)(sess, builder.names, _path, args)
        print('%s: %d objects detected' % (_path, len(results)))
        for r in results:
            print('  %s %.1f%% (%.1f, %.1f)-(%.1f, %.1f)' % r)
        if args.output:
            os.makedirs(args.output, exist_ok=True)
            draw(_path, results, os.path.join(args.output, os.path.basename(_path) + '.png'))


def make_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('path', help='input image path')
    parser.add_argument('-c', '--config', nargs='+', default=['config.ini'], help='config file')
    parser.add_argument('-p', '--preprocess', default='std', choices=sorted(PREPROCESS), help='the preprocess function')
    parser.add_argument('-t', '--threshold', type=float, default=0.3)
    parser.add_argument('--threshold_iou', type=float, default=0.4, help='IoU threshold')
    parser.add_argument('-e', '--exts', nargs='+', default=['.jpg', '.png'])
    parser.add_argument('--level', default='info', help='logging level')
    parser.add_argument('--output', help='directory for annotated images (the reference opens a matplotlib window instead)')
    parser.add_argument('--dtype', default=None, choices=['bf16', 'f32', 'int8'], help="'int8': post-training quantised inference (needs a calibration)")
    parser.add_argument('--calibration', default=None, help='--dtype int8: the file quantize.py wrote (default: calibration.npz in the logdir)')
    parser.add_argument('--ema', action='store_true', help='use the moving averages of the weights a run with [mi355x] ema_decay keeps in its checkpoints')
    options.add_flags(parser, ('nms', ('sigma', 'nms_sigma'), 'tta', 'tta_iou'))         # None: the key, or its default, decides
    return parser.parse_args(argv)


if __name__ == '__main__':
    args = make_args()
    config = configparser.ConfigParser()
    utils.load_config(config, args.config)
    logging.basicConfig()
    if args.level:
        logging.getLogger().setLevel(args.level.upper())
    main()
