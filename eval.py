#!/usr/bin/env python
"""eval.py -- mean average precision of a checkpoint on MI355X (PASCAL VOC or COCO protocol; new work, the reference has no evaluator):

    python eval.py -c config.ini config/yolo2/darknet-20.ini -p val -b 64 -t 0.005 --threshold_iou 0.45 --iou 0.5 --mode all --json out.json
    python eval.py -c config.ini config/yolo2/darknet-80.ini -p val -b 64 -t 0.005 --mode all --protocol coco --json out.json

The dataset sits in HBM; resize, forward (moving-average BN), decode, NMS, matching against the ground truth, the per-class sort and
both VOC metrics (11-point `voc07`, area `voc12`) run on the GPU.  Restores the latest checkpoint of utils.get_logdir(config) exactly
as detect.py does.  ``--data cache`` reads the ``-p`` profiles of the reference's TFRecord cache (which has no `difficult` flag: every
box counts), ``--data file.npz`` the raw-object layout train.py accepts plus an optional ``objects_difficult``, ``--data synthetic`` a
seeded generator.  Images are resized by the device's TF-style bilinear kernel, as in training -- not by PIL as in detect.py.
``--protocol coco`` prints COCO's twelve numbers (AP@[.5:.95], AP50, AP75, AP by area, AR by detection limit and by area) instead.  A
.npz file may bring ``objects_crowd`` and ``objects_area``; the reference's cache has no crowd flag (utils/data/cache.py:127 reads
crowd annotations as ordinary boxes), so with ``--data cache`` every box counts and its area is its box area.
``--sizes SPEC`` evaluates the one checkpoint at several input sizes (YOLO9000, table 3): restored once, the dataset uploaded once, one table
under a ``size WxH`` line per size, a closing table (size, the two mean APs, milliseconds per batch by HIP events), ``by_size`` in the JSON.
Import-safe."""
import argparse
import configparser
import json
import logging
import os

from yolo_tf_amd import options, utils

PREPROCESS = {'std': 0, 'darknet': 1}


def load_data(args, config, classes):
    """(images, objects, difficult or None, crowd or None, area or None) of the chosen source."""
    from yolo_tf_amd import evaluate
    if args.data == 'synthetic':
        return evaluate.synthetic_dataset(args.images, classes, seed=args.seed) + (None, None)
    if args.data == 'cache':
        from yolo_tf_amd.utils import tfrecord
        cachedir = utils.get_cachedir(config)
        paths = [os.path.join(cachedir, profile + '.tfrecord') for profile in args.profile]
        logging.info('loading ' + ', '.join(paths))
        images, objects = tfrecord.load_dataset(paths, limit=args.limit)
        return images, objects, None, None, None
    fields = evaluate.load_npz(os.path.expanduser(os.path.expandvars(args.data)), coco=True)
    if args.limit is not None:
        fields = tuple(f if f is None else f[:args.limit] for f in fields)
    return fields


def main():
    from yolo_tf_amd import checkpoint, evaluate, tf_checkpoint
    from yolo_tf_amd.session import DetectSession
    model = config.get('config', 'model')
    yolo = __import__('yolo_tf_amd.model.' + model, fromlist=['Builder'])
    utils.ensure_names(config)
    builder = yolo.Builder(args, config)
    builder(None)
    dtype = options.read(config, 'dtype', args.dtype or None)
    args.nms, args.sigma = utils.nms_options(args, config)      # --nms / --sigma, else [mi355x] nms / nms_sigma, else hard
    logdir = utils.get_logdir(config)
    calibration = None
    if dtype == 'int8':       # post-training quantised inference: the scales quantize.py measured for this checkpoint
        from yolo_tf_amd import quant
        calibration = quant.calibration_path(logdir, args.calibration)
    sizes = None
    if args.sizes is not None:
        # one set of weights at several input sizes (YOLO9000, table 3): restored once, evaluated once per size
        from yolo_tf_amd import multiscale
        if model == 'yolo':
            raise ValueError('--sizes %r: the fully connected head of the YOLO (v1) family fixes the input size' % args.sizes)
        try:
            sizes = multiscale.parse_sizes(args.sizes, *utils.get_downsampling(config))
        except ValueError as e:
            raise ValueError('--sizes %r: %s' % (args.sizes, e))
        if not sizes:
            raise ValueError('--sizes %r names no size' % args.sizes)
        multiscale.check_nested(sorted(set(sizes) | {(builder.width, builder.height)}), '--sizes %r' % args.sizes)
        if dtype == 'int8':
            raise ValueError('--sizes with --dtype int8: quantised inference binds one input size; run eval.py once per size')
    # test-time augmentation: --tta / --tta_iou, else [mi355x] tta / tta_iou; views fused on the device into ONE result
    from yolo_tf_amd import tta
    spec, args.tta_iou = tta.options(config, args.tta, args.tta_iou)
    views = tta.parse_views(spec, (builder.width, builder.height), *(utils.get_downsampling(config) if model != 'yolo' else (1, 1)))
    if views and sizes is not None:
        raise ValueError('--tta %r with --sizes %r: --sizes makes one table per input size, --tta fuses its views into one result; give one of them'
                         % (spec, args.sizes))
    args.tta = tta.describe(views) if views else None
    if views:
        logging.info('test-time augmentation: views %s, fused at IoU %g' % (args.tta, args.tta_iou))
        if not tta.flip_only(views):
            from yolo_tf_amd import multiscale
            multiscale.check_nested(tta.view_sizes(views), '--tta %r' % spec)
    sess = DetectSession(builder, args.batch_size, dtype=dtype, calibration=calibration, sizes=sizes, tta=views or None, tta_rows='evaluation' if views else None)
    model_path = checkpoint.latest_checkpoint(logdir)
    tf_path = None if model_path else tf_checkpoint.latest_checkpoint(logdir)
    if model_path is None and tf_path is None:
        raise FileNotFoundError('no checkpoint in ' + logdir)
    logging.info('load ' + (model_path or tf_path))
    step = checkpoint.restore(model_path, engine=sess.engine, ema=args.ema) if model_path else tf_checkpoint.restore(tf_path, engine=sess.engine, ema=args.ema)
    logging.info('global_step=%d' % step)
    images, objects, difficult, crowd, area = load_data(args, config, len(builder.names))
    m = sess.model
    data = evaluate.EvalData(images, objects, args.batch_size, builder.width, builder.height, m.cell_width, m.cell_height, difficult=difficult,
                             crowd=crowd, area=area, input_sizes=sizes if not views or tta.flip_only(views) else tta.view_sizes(views))
    extra = dict(names=list(builder.names), images=len(images), checkpoint=model_path or tf_path, global_step=int(step), calibration=calibration, ema=bool(args.ema),
                 config={k: getattr(args, k) for k in ('config', 'profile', 'data', 'batch_size', 'threshold', 'threshold_iou', 'iou', 'mode', 'protocol',
                                                       'preprocess', 'dtype', 'limit', 'images', 'seed', 'nms', 'sigma', 'tta', 'tta_iou')})

    def run(on_batch=None):
        return evaluate.evaluate(builder, sess, data, mode=args.mode, threshold=args.threshold, threshold_iou=args.threshold_iou, iou=args.iou,
                                 preprocess_mode=PREPROCESS[args.preprocess], max_records=args.max_records, protocol=args.protocol, on_batch=on_batch,
                                 nms=args.nms, sigma=args.sigma, tta=views or None, fuse_iou=args.tta_iou)
    if sizes is None:
        result = run()
        out = report(args, builder, result)
        if args.json:
            write_json(args.json, dict(out, **extra))
        return result
    import torch
    by_size, ms, results = {}, {}, {}
    for w, h in sizes:
        key = '%dx%d' % (w, h)
        sess.set_size(w, h)
        data.set_size(w, h)
        # HIP events around the batches (resize, forward, decode, NMS, matching), not around the final sort and download; the first
        # batch at a size builds that size's plans, which is part of the figure
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        result = run(on_batch=lambda *a: end.record())
        end.synchronize()
        ms[key] = start.elapsed_time(end) / len(data)
        print('size ' + key)
        by_size[key] = report(args, builder, result)
        results[key] = result
    coco = args.protocol == 'coco'
    print(('%-10s %8s %8s %12s' % ('size', 'AP', 'AP50', 'ms/batch')) if coco else ('%-10s %8s %8s %12s' % ('size', 'mAP07', 'mAP12', 'ms/batch')))
    for key, result in results.items():
        a, b = (result['stats'][0], result['stats'][1]) if coco else (result['mAP07'], result['mAP12'])
        print('%-10s %8.4f %8.4f %12.3f' % (key, a, b, ms[key]))
    if args.json:
        write_json(args.json, dict(extra, sizes=list(by_size), by_size=by_size, ms_per_batch=ms))
    return results


def report(args, builder, result):
    """Prints one evaluation's table and returns what --json writes of it."""
    from yolo_tf_amd import evaluate
    if args.protocol == 'coco':
        for name, v in zip(evaluate.COCO_STAT_NAMES, result['stats']):
            print('%s = %0.3f' % (name, v))
        return dict(stats=result['stats'], stat_names=[n.strip() for n in evaluate.COCO_STAT_NAMES], detections=result['detections'],
                    **{k: result[k].tolist() for k in ('ap', 'recall', 'npig')})
    print('%-16s %8s %8s %6s %6s %8s' % ('class', 'ap07', 'ap12', 'npos', 'tp', 'fp'))
    for i, name in enumerate(builder.names):
        print('%-16s %8.4f %8.4f %6d %6d %8d' % (name, result['ap07'][i], result['ap12'][i], result['npos'][i], result['tp'][i], result['fp'][i]))
    print('mAP07 %.4f' % result['mAP07'])
    print('mAP12 %.4f' % result['mAP12'])
    return dict(result)


def write_json(path, out):
    with open(os.path.expanduser(os.path.expandvars(path)), 'w') as f:
        json.dump(out, f, indent=1)          # (NaN of a class without ground truth is written as NaN, which Python's json reads back)


def make_args(argv=None):
    parser = argparse.ArgumentParser(description='VOC mean average precision of the latest checkpoint, evaluated on the GPU')
    parser.add_argument('-c', '--config', nargs='+', default=['config.ini'], help='config file')
    parser.add_argument('-p', '--profile', nargs='+', default=['val'], help='dataset profiles of the cache (--data cache)')
    parser.add_argument('--data', default='cache', help="'cache' (the reference's TFRecord cache), 'synthetic' or a .npz file with raw objects")
    parser.add_argument('-b', '--batch_size', type=int, default=64)
    parser.add_argument('-t', '--threshold', type=float, default=0.005, help='score threshold of a detection')
    parser.add_argument('--threshold_iou', type=float, default=0.45, help='IoU threshold of the NMS')
    parser.add_argument('--iou', type=float, default=0.5, help='IoU a detection needs (strictly above) to match a ground truth box')
    parser.add_argument('--mode', default='detect', choices=['detect', 'all'],
                        help="'detect': one detection per box, its arg-max class (detect.py); 'all': one per (box, class) (Darknet valid)")
    parser.add_argument('--protocol', default='voc', choices=['voc', 'coco'],
                        help="'voc': the two PASCAL VOC average precisions at --iou; 'coco': COCO's twelve numbers (IoU .5:.95, area ranges, "
                             "detection limits 1 / 10 / 100; --iou is unused).  With --data cache no box is crowd: the reference's cache reads crowd "
                             "annotations as ordinary boxes")
    parser.add_argument('--preprocess', default='std', choices=sorted(PREPROCESS), help='the preprocess function')
    parser.add_argument('--json', help='write the result, the configuration, the checkpoint path and the global step here')
    parser.add_argument('--limit', type=int, default=None, help='evaluate only the first images')
    parser.add_argument('--images', type=int, default=32, help='--data synthetic: number of images')
    parser.add_argument('--seed', type=int, default=0, help='--data synthetic: seed')
    parser.add_argument('--max_records', type=int, default=None, help='capacity of the record buffer (default: the worst case of the mode)')
    parser.add_argument('--dtype', default=None, choices=['bf16', 'f32', 'int8'], help="'int8': post-training quantised inference (needs a calibration)")
    parser.add_argument('--calibration', default=None, help='--dtype int8: the file quantize.py wrote (default: calibration.npz in the logdir)')
    parser.add_argument('--sizes', default=None, help="evaluate the one checkpoint at several input sizes: entries S, WxH or LO-HI (squares in steps of the "
                        "network's stride) separated by spaces or commas, e.g. '320-608'; prints one table per size and a closing one, --json gets by_size")
    parser.add_argument('--ema', action='store_true', help='use the moving averages of the weights a run with [mi355x] ema_decay keeps in its checkpoints')
    options.add_flags(parser, ('nms', ('sigma', 'nms_sigma'), 'tta', 'tta_iou'))         # None: the key, or its default, decides
    parser.add_argument('--level', default='info', help='logging level')
    return parser.parse_args(argv)


if __name__ == '__main__':
    args = make_args()
    config = configparser.ConfigParser()
    utils.load_config(config, args.config)
    logging.basicConfig()
    if args.level:
        logging.getLogger().setLevel(args.level.upper())
    main()
