#!/usr/bin/env python
"""anchors.py -- dimension clusters on MI355X: fits the YOLOv2 anchors of a dataset (new work; the reference lists "Dimension cluster" as
an unchecked roadmap item, README.md:88, and ships two constant anchor files):

    python anchors.py -c config.ini config/yolo2/darknet-20.ini -p train val -k 5 -o my_anchors.tsv
    python anchors.py -c config.ini config/yolo2/darknet-20.ini --data synthetic --boxes 100000 -k 1-16 --restarts 16 --json sweep.json
    python anchors.py -c config.ini config/yolo2/darknet-20.ini -p train --score config/yolo2/anchors/voc.tsv

k-means over the ground truth boxes' (w, h) in grid-cell units with distance 1 - IoU (YOLO9000, section 2), every k of the sweep times
every restart in the same kernel launches.  The grid is the configured input size over the model's downsampling, exactly as train.py
derives it.  ``--data cache`` reads the ``-p`` profiles of the reference's TFRecord cache (image shapes and boxes only, no image is
decoded), ``--data file.npz`` the raw-object layout train.py accepts, ``--data synthetic`` a seeded generator.  Prints one line per k:
k, the best restart's average IoU, its iterations, its empty clusters.  ``-o`` receives the anchors of the single k, or of ``--pick K``
of a range; ``[yolo2] anchors`` of a config file then points at it.  ``--score`` only reports how well a given anchor file fits the boxes.
Import-safe."""
import argparse
import configparser
import json
import logging
import os

from yolo_tf_amd import utils


def parse_ks(text):
    """'5' -> [5]; '1-16' -> [1, ..., 16]."""
    lo, sep, hi = text.partition('-')
    try:
        ks = list(range(int(lo), int(hi) + 1)) if sep else [int(lo)]
    except ValueError:
        raise argparse.ArgumentTypeError('-k takes a number or a-b, not %r' % text)
    if not ks or ks[0] < 1 or ks[-1] > 32:
        raise argparse.ArgumentTypeError('-k: 1 <= k <= 32 (and a <= b), not %r' % text)
    return ks


def load_boxes(args, config):
    from yolo_tf_amd import anchors
    section = config.get('config', 'model')
    width, height = config.getint(section, 'width'), config.getint(section, 'height')
    cells_x, cells_y = utils.calc_cell_width_height(config, width, height)
    paths = None
    if args.data == 'cache':
        cachedir = utils.get_cachedir(config)
        paths = [os.path.join(cachedir, profile + '.tfrecord') for profile in args.profile]
        logging.info('loading ' + ', '.join(paths))
    boxes = anchors.read_boxes(args.data, cells_x, cells_y, cache_paths=paths, n=args.boxes, seed=args.seed)
    logging.info('%d boxes on a %d x %d grid' % (len(boxes), cells_x, cells_y))
    return boxes, (cells_x, cells_y)


def main():
    from yolo_tf_amd import anchors
    boxes, cells = load_boxes(args, config)
    dc = anchors.DimensionClusters(boxes)
    extra = dict(boxes=len(boxes), cells=list(cells),
                 config={k: getattr(args, k) for k in ('config', 'profile', 'data', 'k', 'restarts', 'max_iter', 'seed', 'pick', 'score')})
    if args.score:
        given = utils.read_anchors(args.score)
        avg, counts = dc.score(given)
        print('%s: k %d  avg IoU %.6f  empty %d' % (args.score, len(given), avg, int((counts == 0).sum())))
        out = dict(extra, anchors=given.tolist(), avg_iou=avg, counts=counts.tolist())
    else:
        result = dc.fit(args.k, restarts=args.restarts, max_iter=args.max_iter, seed=args.seed)
        print('%3s %10s %10s %6s' % ('k', 'avg IoU', 'iterations', 'empty'))
        for k in args.k:
            r = result[k]
            print('%3d %10.6f %10d %6d%s' % (k, r['avg_iou'], r['iterations'], int((r['counts'] == 0).sum()), '' if r['converged'] else '  (not converged)'))
        pick = args.k[0] if len(args.k) == 1 else args.pick
        if args.output and pick is not None:
            anchors.write_anchors(args.output, result[pick]['anchors'])
            logging.info('k = %d anchors written to %s' % (pick, args.output))
        out = dict(extra, sweep=[dict(k=k, anchors=result[k]['anchors'].tolist(), avg_iou=result[k]['avg_iou'], counts=result[k]['counts'].tolist(),
                                      iterations=result[k]['iterations'], converged=result[k]['converged'], restart=result[k]['restart'],
                                      restart_avg_iou=result[k]['restart_avg_iou']) for k in args.k])
    if args.json:
        with open(os.path.expanduser(os.path.expandvars(args.json)), 'w') as f:
            json.dump(out, f, indent=1)
    return out


def make_args(argv=None):
    parser = argparse.ArgumentParser(description='dimension clusters: YOLOv2 anchors of a dataset, fitted on the GPU')
    parser.add_argument('-c', '--config', nargs='+', default=['config.ini'], help='config file')
    parser.add_argument('-p', '--profile', nargs='+', default=['train', 'val'], help='dataset profiles of the cache (--data cache)')
    parser.add_argument('--data', default='cache', help="'cache' (the reference's TFRecord cache), 'synthetic' or a .npz file with raw objects")
    parser.add_argument('-k', type=parse_ks, default=[5], help='number of anchors: a number, or a-b for a sweep (1 <= k <= 32)')
    parser.add_argument('--restarts', type=int, default=16, help='random initialisations per k; the best average IoU wins')
    parser.add_argument('--max_iter', type=int, default=500, help='updates after which a job that has not reached its fixed point is cut off')
    parser.add_argument('--seed', type=int, default=0, help='seed of the initialisations (and of --data synthetic)')
    parser.add_argument('-o', '--output', help='anchor TSV to write: required with a single k; with a range it receives the anchors of --pick')
    parser.add_argument('--pick', type=int, default=None, help='with a range of k: the k whose anchors -o receives')
    parser.add_argument('--json', help='write the whole sweep (or the score) here')
    parser.add_argument('--score', help='an anchor TSV: only report its average IoU and counts on the boxes')
    parser.add_argument('--boxes', type=int, default=100000, help='--data synthetic: number of boxes')
    parser.add_argument('--level', default='info', help='logging level')
    args = parser.parse_args(argv)
    if not args.score:
        if len(args.k) == 1 and not args.output:
            parser.error('-o is required with a single k')
        if args.pick is not None and (len(args.k) == 1 or args.pick not in args.k or not args.output):
            parser.error('--pick names a k of the range -k a-b and needs -o')
    return args


if __name__ == '__main__':
    args = make_args()
    config = configparser.ConfigParser()
    utils.load_config(config, args.config)
    logging.basicConfig()
    if args.level:
        logging.getLogger().setLevel(args.level.upper())
    main()
