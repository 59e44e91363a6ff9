"""Post-training int8 calibration of the latest checkpoint: runs the bf16 network over a few batches, measures the abs-max of every
tensor the int8 network stores, and writes the per-tensor scales next to the checkpoint.

    python quantize.py -c config.ini config/yolo2/darknet-20.ini -p train --batches 8 -b 32 [--data synthetic|file.npz|cache] -o calibration.npz

--method percentile | mse | entropy clips instead of taking the abs-max: a second pass over the same batches fills one histogram of |x| per
scale class, the method picks a threshold from it, and one line per class says what it did (--percentile P: default 99.99).

Afterwards `detect.py --dtype int8` and `eval.py --dtype int8` run the quantised network (--calibration FILE, default: the logdir's file).
"""
import argparse
import configparser
import logging
import os

from yolo_tf_amd import utils

PREPROCESS = {'std': 0, 'darknet': 1}


def main():
    from eval import load_data
    from yolo_tf_amd import checkpoint, evaluate, quant, tf_checkpoint
    from yolo_tf_amd.session import DetectSession
    model = config.get('config', 'model')
    yolo = __import__('yolo_tf_amd.model.' + model, fromlist=['Builder'])
    utils.ensure_names(config)
    builder = yolo.Builder(args, config)
    builder(None)
    if getattr(builder, 'family', 'yolo2') == 'yolo':
        raise NotImplementedError('int8 inference covers the YOLOv2 family: the YOLO (v1) fully connected head is not quantised')
    sess = DetectSession(builder, args.batch_size, dtype='bf16')
    logdir = utils.get_logdir(config)
    model_path = checkpoint.latest_checkpoint(logdir)
    tf_path = None if model_path else tf_checkpoint.latest_checkpoint(logdir)
    if model_path is None and tf_path is None:
        raise FileNotFoundError('no checkpoint in ' + logdir)
    logging.info('load ' + (model_path or tf_path))
    step = checkpoint.restore(model_path, engine=sess.engine, ema=args.ema) if model_path else tf_checkpoint.restore(tf_path, engine=sess.engine, ema=args.ema)
    images, objects = load_data(args, config, len(builder.names))[:2]
    m = sess.model
    data = evaluate.EvalData(images, objects, args.batch_size, builder.width, builder.height, m.cell_width, m.cell_height)
    cal = quant.Calibrator(sess, method=args.method, percentile=args.percentile)
    for batch, _, _, _ in data:
        if cal.batches >= args.batches:
            break
        cal.observe(batch, PREPROCESS[args.preprocess])
    if args.method != 'absmax':
        for batch, _, _, _ in data:
            if cal.hist_batches >= cal.batches:
                break
            cal.observe_histogram(batch, PREPROCESS[args.preprocess])
    calibration = cal.finish()
    if args.method != 'absmax':
        for r in cal.report:
            print('%s: abs-max %.6g, %s threshold %.6g (%.4f of it), %.4f %% of the values clipped, SQNR estimate %.2f dB (abs-max: %.2f dB)' % (
                ' '.join(r['members']), r['amax'], args.method, r['threshold'], r['threshold'] / r['amax'], 100 * r['clipped'], r['sqnr_db'],
                r['sqnr_db_absmax']))
    out = os.path.expanduser(os.path.expandvars(args.output)) if args.output else os.path.join(logdir, quant.CALIBRATION_FILE)
    calibration.save(out)
    print('global_step=%d: %d batches of %d images, %d tensors in %d scale classes -> %s' % (
        step, cal.batches, args.batch_size, len(calibration.scales), len(cal.plan.classes), out))
    return out


def make_args(argv=None):
    parser = argparse.ArgumentParser(description='int8 calibration of the latest checkpoint (abs-max over a few batches, on the GPU)')
    parser.add_argument('-c', '--config', nargs='+', default=['config.ini'], help='config file')
    parser.add_argument('-p', '--profile', nargs='+', default=['train'], help='dataset profiles of the cache (--data cache)')
    parser.add_argument('--data', default='cache', help="'cache' (the reference's TFRecord cache), 'synthetic' or a .npz file with raw objects")
    parser.add_argument('-b', '--batch_size', type=int, default=32)
    parser.add_argument('--batches', type=int, default=8, help='number of calibration batches')
    parser.add_argument('--method', default='absmax', choices=['absmax', 'percentile', 'mse', 'entropy'],
                        help='how a scale class gets its range: its abs-max, or a clipping threshold chosen from a histogram (a second pass over the batches)')
    parser.add_argument('--percentile', type=float, default=99.99, help='--method percentile: the share of the values, in percent, the range keeps')
    parser.add_argument('--preprocess', default='std', choices=sorted(PREPROCESS), help='the preprocess function detection will use')
    parser.add_argument('-o', '--output', default=None, help='calibration file (default: calibration.npz in the logdir, beside the checkpoint)')
    parser.add_argument('--images', type=int, default=None, help='--data synthetic: number of images (default: batches * batch size)')
    parser.add_argument('--seed', type=int, default=0, help='--data synthetic: seed')
    parser.add_argument('--ema', action='store_true', help='use the moving averages of the weights a run with [mi355x] ema_decay keeps in its checkpoints')
    parser.add_argument('--level', default='info', help='logging level')
    args = parser.parse_args(argv)
    args.limit = args.batches * args.batch_size
    if args.images is None:
        args.images = args.limit
    return args


if __name__ == '__main__':
    args = make_args()
    config = configparser.ConfigParser()
    utils.load_config(config, args.config)
    logging.basicConfig()
    if args.level:
        logging.getLogger().setLevel(args.level.upper())
    main()
