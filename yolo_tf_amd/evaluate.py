"""On-device evaluation of a detector: PASCAL VOC average precision and COCO's AP / AR (new work: the reference has no evaluator).

``Evaluator`` scores what a ``DetectSession`` leaves on the device after ``detect()``: ``add`` matches one batch against its ground
truth and appends (score, class, TP / FP / ignored, image, box) records to a buffer in HBM without synchronising, ``result`` sorts the
records per class on the device, integrates both VOC metrics there and downloads one small block.  ``EvalData`` walks a dataset held
in HBM in order, ``evaluate`` ties the two to a session.  The rules (include/yolo2_hip.h, section "evaluation") are the VOC devkit's.
``CocoEvaluator`` has the same surface and follows pycocotools' COCOeval for boxes (section "evaluation, COCO protocol": 101 recall
points, IoU 0.5:0.95, area ranges, detection limits, greedy matching to the best box that is still free), with two stated limits: IoU is
computed in f32, and a ground truth box's area is its box area unless the data brings the segmentation's.
"""
import math

import numpy as np
import torch

from . import ops
from ._lib import HipKernelError, query
from .utils.augment import FLIP as AUGMENT_FLIP
from .utils.augment import AugmentConfig, DeviceInputPipeline

RECORD_DTYPE = np.dtype([('score', '<f4'), ('image', '<i4'), ('box', '<i4'), ('class_flag', '<u4')])      # yolo2_eval_record
FP, TP, IGNORED = 0, 1, 2


class Evaluator(object):
    """VOC average precision of detections, accumulated over batches on the device.

    classes: number of classes C.  max_records: capacity of the record buffer (16 bytes each); a dataset of I images of N boxes
    needs at most I * N records in mode 'detect' and I * N * C in mode 'all'.  mode: 'detect' = one detection per box (class = first
    arg-max of its scores; what detect.py prints), 'all' = one per (box, class) above the threshold (what Darknet's `valid` emits and
    published VOC numbers use).  threshold: score threshold (strict >).  iou_threshold: a detection matches when IoU > it (strict).
    keep_curve: also keep the sorted records and the cumulative TP / FP counts on the device (``curve()``)."""

    def __init__(self, classes, max_records, mode='detect', threshold=0.005, iou_threshold=0.5, device=None, keep_curve=False):
        if mode not in ops.EVAL_MODES:
            raise ValueError("mode must be 'detect' or 'all', not %r" % (mode,))
        self.C, self.max_records, self.mode = int(classes), int(max_records), mode
        self.threshold, self.iou_threshold = float(threshold), float(iou_threshold)
        if self.C <= 0 or self.max_records <= 0:
            raise ValueError('classes and max_records must be positive')
        dev = torch.device('cuda') if device is None else device
        self.records = torch.zeros(int(query('yolo2_eval_record_bytes', self.max_records)), dtype=torch.uint8, device=dev)
        self.state = torch.zeros(ops.EVAL_STATE_WORDS, dtype=torch.int64, device=dev)
        self.npos = torch.zeros(self.C, dtype=torch.int32, device=dev)
        self.results = torch.zeros(int(query('yolo2_eval_result_bytes', self.C)) // 8, dtype=torch.int64, device=dev)
        self.ws = None                    # the sort's workspace (two record buffers): allocated by the first result()
        self.collect_ws = None
        self.keep_curve = keep_curve
        self.sorted = self.cum_tp = self.cum_fp = None
        self.n_images, self.N = 0, 1

    def reset(self):
        self.state.zero_()
        self.npos.zero_()
        self.n_images, self.N = 0, 1

    def add(self, conf, xy_min, xy_max, gt_class, gt_box, gt_difficult, gt_first, image_base, n_valid=None):
        """conf [B,N,C] f32 after NMS, xy_min / xy_max [B,N,2] f32 (cell units); gt_class [G] int32, gt_box [G,4] f32 in the same cell
        units, gt_difficult [G] uint8, gt_first [B+1] int32 (offsets per image): device tensors (at least one element each, whatever
        gt_first says).  image_base: dataset index of the batch's first image; images b >= n_valid are padding.  No synchronisation."""
        B, N, C = conf.shape
        if C != self.C:
            raise ValueError('conf has %d classes, the evaluator %d' % (C, self.C))
        n_valid = B if n_valid is None else int(n_valid)
        if self.collect_ws is None or self.collect_ws.numel() < B:
            self.collect_ws = torch.zeros(ops.workspace_bytes('eval_collect', B) // 4, dtype=torch.int32, device=conf.device)
        ops.eval_collect(conf, xy_min, xy_max, gt_class, gt_box, gt_difficult, gt_first, int(gt_class.numel()), B, N, C, n_valid, int(image_base),
                         ops.EVAL_MODES[self.mode], self.threshold, self.iou_threshold, self.records, self.max_records, self.state, self.npos,
                         self.collect_ws)
        self.n_images = max(self.n_images, int(image_base) + n_valid)
        self.N = max(self.N, N)

    def result(self):
        """Sorts and integrates on the device, then one synchronisation and one small download.  Returns {'ap07', 'ap12' (lists of
        float, NaN for a class without ground truth), 'npos', 'tp', 'fp', 'ignored' (lists of int), 'mAP07', 'mAP12' (means over the
        classes that have ground truth; NaN if none), 'detections' (records, ignored ones included)}.  Raises HipKernelError naming the
        needed count when max_records was too small."""
        dev = self.records.device
        if self.ws is None:
            self.ws = torch.zeros(ops.workspace_bytes('eval', self.max_records, self.C), dtype=torch.uint8, device=dev)
        if self.keep_curve and self.sorted is None:
            self.sorted = torch.zeros_like(self.records)
            self.cum_tp = torch.zeros(self.max_records, dtype=torch.int32, device=dev)
            self.cum_fp = torch.zeros(self.max_records, dtype=torch.int32, device=dev)
        ops.eval_finalize(self.records, self.max_records, self.state, self.npos, self.C, max(self.n_images, 1), self.N, self.ws, self.results,
                          self.sorted, self.cum_tp, self.cum_fp)
        words = self.results.cpu().numpy()                # the synchronisation and the download
        C = self.C
        held, needed, errors = (int(v) for v in words[6 * C:6 * C + 3])
        if errors & 1:
            raise HipKernelError('eval: a ground truth class id is outside [0, %d)' % C)
        if errors & 2:
            raise HipKernelError('eval: gt_first is not ascending inside the ground truth arrays, or an image has more than 512 boxes')
        if errors & 4:
            raise HipKernelError('eval: a record names an image, box or class outside the evaluated range')
        if needed > self.max_records:
            raise HipKernelError('eval: the record buffer holds %d records, %d are needed: raise max_records' % (self.max_records, needed))
        ap = words[:2 * C].view(np.float64)
        out = {'ap07': [float(v) for v in ap[:C]], 'ap12': [float(v) for v in ap[C:]]}
        for i, k in enumerate(('npos', 'tp', 'fp', 'ignored')):
            out[k] = [int(v) for v in words[(2 + i) * C:(3 + i) * C]]
        for k in ('07', '12'):
            vals = [v for v in out['ap' + k] if not math.isnan(v)]
            out['mAP' + k] = sum(vals) / len(vals) if vals else float('nan')
        out['detections'] = needed
        self.held = held
        return out

    def records_numpy(self):
        """The appended records (download; tests and tools)."""
        n = min(int(self.state[0].item()), self.max_records)
        return self.records.cpu().numpy().view(RECORD_DTYPE)[:n].copy()

    def curve(self):
        """After result() with keep_curve: (sorted records, cumulative TP, cumulative FP) as NumPy arrays; the records are class-major,
        the ignored ones last, and the counts restart in every class: points of the precision / recall curves."""
        n = self.held
        return self.sorted.cpu().numpy().view(RECORD_DTYPE)[:n].copy(), self.cum_tp.cpu().numpy()[:n].copy(), self.cum_fp.cpu().numpy()[:n].copy()


COCO_RECORD_DTYPE = np.dtype([('score', '<f4'), ('image', '<i4'), ('box', '<i4'), ('class', '<i4'), ('rank', '<i4'), ('reserved', '<u4'),
                              ('matched', '<u8'), ('ignored', '<u8')])      # yolo2_eval_coco_record
COCO_AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))      # all, small, medium, large
COCO_STAT_NAMES = (
    ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ]',
    ' Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ]',
    ' Average Precision  (AP) @[ IoU=0.75      | area=   all | maxDets=100 ]',
    ' Average Precision  (AP) @[ IoU=0.50:0.95 | area= small | maxDets=100 ]',
    ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=medium | maxDets=100 ]',
    ' Average Precision  (AP) @[ IoU=0.50:0.95 | area= large | maxDets=100 ]',
    ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ]',
    ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets= 10 ]',
    ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ]',
    ' Average Recall     (AR) @[ IoU=0.50:0.95 | area= small | maxDets=100 ]',
    ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=medium | maxDets=100 ]',
    ' Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ]')


def coco_slices(areas, max_dets):
    """The (area range, detection limit) pairs the twelve numbers need: range 0 under the limits 1, 10 and 100 that do not exceed
    max_dets (and max_dets itself), every other range under max_dets."""
    limits = sorted(set(l for l in (1, 10, 100) if l < max_dets) | {max_dets})[-3:]
    return [(0, l) for l in limits] + [(a, max_dets) for a in range(1, areas)]


def coco_stats(ap, recall, iou_thresholds, slices):
    """COCO's stats[0..11] from ap / recall [S,T,C]: means over the entries that are not -1 (-1 if none, or if the tables lack the
    slice or the threshold).  0: AP of range 0 under its largest limit; 1, 2: the same at the thresholds equal to float32(.5) and
    float32(.75); 3-5: AP of ranges 1-3; 6-8: AR of range 0 under its limits in ascending order; 9-11: AR of ranges 1-3."""
    slices = [tuple(int(v) for v in s) for s in slices]
    thr = np.asarray(iou_thresholds, np.float32)

    def mean(x, a, limit, t=None):
        if (a, limit) not in slices:
            return -1.0
        v = x[slices.index((a, limit))]
        if t is not None:
            at = np.nonzero(thr == np.float32(t))[0]
            if len(at) == 0:
                return -1.0
            v = v[at[0]]
        v = v[v > -1]
        return float(np.mean(v)) if v.size else -1.0
    own = sorted(l for a, l in slices if a == 0)
    limits = (own + [None] * 3)[:3]                       # (a limit of None names no slice: -1)
    top = max(l for _, l in slices)
    stats = [mean(ap, 0, own[-1] if own else None, t) for t in (None, .5, .75)]
    stats += [mean(ap, a, top) for a in (1, 2, 3)]
    stats += [mean(recall, 0, l) for l in limits]
    stats += [mean(recall, a, top) for a in (1, 2, 3)]
    return stats


class CocoEvaluator(object):
    """COCO AP / AR of detections, accumulated over batches on the device (pycocotools' COCOeval for boxes, with f32 IoU).

    classes, max_records (40 bytes each; an image yields at most max_dets records per class), mode, threshold: as for Evaluator.
    iou_thresholds (at most 10, default .5:.05:.95 as float32), area_ranges (at most 4 (lo, hi) pairs in source pixels squared, default
    COCO's all / small / medium / large), recall_thresholds (at most 101, ascending, default 0:.01:1), max_dets (at most 128, default
    100), slices ((area range index, detection limit) pairs, default ``coco_slices``) are host tables."""

    def __init__(self, classes, max_records, mode='detect', threshold=0.005, iou_thresholds=None, area_ranges=None, recall_thresholds=None,
                 max_dets=100, slices=None, device=None):
        if mode not in ops.EVAL_MODES:
            raise ValueError("mode must be 'detect' or 'all', not %r" % (mode,))
        self.C, self.max_records, self.mode, self.threshold, self.max_dets = int(classes), int(max_records), mode, float(threshold), int(max_dets)
        if self.C <= 0 or self.max_records <= 0:
            raise ValueError('classes and max_records must be positive')
        self.iou_thresholds = np.linspace(.5, .95, 10).astype(np.float32) if iou_thresholds is None else np.asarray(iou_thresholds, np.float32).reshape(-1)
        self.area_ranges = np.asarray(COCO_AREA_RANGES if area_ranges is None else area_ranges, np.float32).reshape(-1, 2)
        self.recall_thresholds = np.linspace(0, 1, 101) if recall_thresholds is None else np.asarray(recall_thresholds, np.float64).reshape(-1)
        self.A, self.T, self.R = len(self.area_ranges), len(self.iou_thresholds), len(self.recall_thresholds)
        self.slices = np.asarray(coco_slices(self.A, self.max_dets) if slices is None else slices, np.int32).reshape(-1, 2)
        self.S = len(self.slices)
        dev = torch.device('cuda') if device is None else device
        self.records = torch.zeros(int(query('yolo2_eval_coco_record_bytes', self.max_records)), dtype=torch.uint8, device=dev)
        self.state = torch.zeros(ops.EVAL_STATE_WORDS, dtype=torch.int64, device=dev)
        self.npig = torch.zeros(max(self.A, 1) * self.C, dtype=torch.int32, device=dev)
        self.results = torch.zeros(max(int(query('yolo2_eval_coco_result_bytes', self.S, self.T, self.A, self.C)) // 8, 1), dtype=torch.int64, device=dev)
        self.ws = self.collect_ws = None
        self.n_images, self.N = 0, 1

    def reset(self):
        self.state.zero_()
        self.npig.zero_()
        self.n_images, self.N = 0, 1

    def add(self, conf, xy_min, xy_max, gt_class, gt_box, gt_area, gt_flags, gt_first, scale, image_base, n_valid=None):
        """As Evaluator.add, plus gt_area [G] f32 (source pixels squared), gt_flags [G] uint8 (bit 0 ignore, bit 1 crowd) and scale
        [B,2] f32 (source pixels per cell, x and y, of each image): device tensors.  No synchronisation."""
        B, N, C = conf.shape
        if C != self.C:
            raise ValueError('conf has %d classes, the evaluator %d' % (C, self.C))
        n_valid = B if n_valid is None else int(n_valid)
        need = ops.workspace_bytes('eval_coco_collect', B, N, C)
        if self.collect_ws is None or self.collect_ws.numel() < need:
            self.collect_ws = torch.zeros(max(need, 1), dtype=torch.uint8, device=conf.device)
        ops.eval_coco_collect(conf, xy_min, xy_max, gt_class, gt_box, gt_area, gt_flags, gt_first, scale, int(gt_class.numel()), B, N, C, n_valid,
                              int(image_base), ops.EVAL_MODES[self.mode], self.threshold, self.area_ranges, self.A, self.iou_thresholds, self.T,
                              self.max_dets, self.records, self.max_records, self.state, self.npig, self.collect_ws)
        self.n_images = max(self.n_images, int(image_base) + n_valid)
        self.N = max(self.N, N)

    def result(self):
        """Sorts and integrates on the device, then one synchronisation and one small download.  Returns {'stats' (COCO's twelve
        numbers, ``coco_stats``), 'ap', 'recall' (float64 arrays [S,T,C]; -1 where the class has no ground truth in the slice's area
        range), 'npig' (int array [A,C]), 'detections' (records)}.  Raises HipKernelError as Evaluator.result does."""
        if self.ws is None:
            self.ws = torch.zeros(ops.workspace_bytes('eval_coco', self.max_records, self.C), dtype=torch.uint8, device=self.records.device)
        ops.eval_coco_finalize(self.records, self.max_records, self.state, self.npig, self.C, max(self.n_images, 1), self.N, self.A, self.T,
                               self.max_dets, self.slices, self.S, self.recall_thresholds, self.R, self.ws, self.results)
        words = self.results.cpu().numpy()                # the synchronisation and the download
        S, T, A, C = self.S, self.T, self.A, self.C
        n = S * T * C
        held, needed, errors = (int(v) for v in words[2 * n + A * C:2 * n + A * C + 3])
        if errors & 1:
            raise HipKernelError('eval: a ground truth class id is outside [0, %d)' % C)
        if errors & 2:
            raise HipKernelError('eval: gt_first is not ascending inside the ground truth arrays, or an image has more than 512 boxes')
        if errors & 4:
            raise HipKernelError('eval: a record names an image, box, class or rank outside the evaluated range')
        if needed > self.max_records:
            raise HipKernelError('eval: the record buffer holds %d records, %d are needed: raise max_records' % (self.max_records, needed))
        ap = words[:n].view(np.float64).reshape(S, T, C).copy()
        recall = words[n:2 * n].view(np.float64).reshape(S, T, C).copy()
        self.held = held
        return {'stats': coco_stats(ap, recall, self.iou_thresholds, self.slices), 'ap': ap, 'recall': recall,
                'npig': words[2 * n:2 * n + A * C].reshape(A, C).copy(), 'detections': needed}

    def records_numpy(self):
        """The appended records (download; tests and tools)."""
        n = min(int(self.state[0].item()), self.max_records)
        return self.records.cpu().numpy().view(COCO_RECORD_DTYPE)[:n].copy()


class EvalData(object):
    """A sequential, unshuffled, unaugmented walk over a dataset held in HBM.

    images: list of uint8 [h, w, 3] arrays (any sizes); objects: list of (classes int [K], boxes float [K,4] in pixels of the image:
    xmin, ymin, xmax, ymax); difficult: list of [K] flags or None (all zero: the reference's dataset cache has no such field).
    crowd: list of [K] flags or None; area: list of [K] areas in source pixels squared or None (the box area): the COCO protocol's.
    Iterating yields (image batch f32 [B,H,W,3] 0..255, (gt_class, gt_box, gt_difficult, gt_first) device tensors with the boxes in
    CELL units, image_base, n_valid).  The last batch is padded to B with copies of the dataset's first image that own no ground
    truth; n_valid says how many images count.  ``batches('coco')`` yields the ground truth as (gt_class, gt_box, gt_area, gt_flags,
    gt_first, scale) instead: flags = difficult | crowd << 1, scale [B,2] = source pixels per cell of each image.

    The resize is the device's TF-style bilinear one (yolo2_augment_images with the full-image crop and no flags), the one training
    sees.  It is NOT the PIL resize detect.py applies to a file, so scores can differ slightly from what detect.py prints."""

    def __init__(self, images, objects, batch, width, height, cell_width, cell_height, difficult=None, crowd=None, area=None, input_sizes=None):
        """``input_sizes``: optional list of (width, height) the data can be walked at (``set_size``; width x height comes first): the
        decoded dataset is uploaded once, the batch buffer is allocated for the largest of them, the ground truth in cell units is
        recomputed for the grid of each (the network's stride is what width / cell_width and height / cell_height say)."""
        # the training pipeline with every augmentation disabled: its draw() then yields the full-image crop and no flags
        self.pipe = DeviceInputPipeline(images, objects, batch, width, height, None, cell_width, cell_height, config=AugmentConfig(None),
                                        sizes=input_sizes)
        self.B, self.sizes = batch, self.pipe.sizes
        self._objects, self._difficult = objects, difficult
        self.gt = gt_in_cells(objects, self.sizes, cell_width, cell_height, difficult)
        self.area, self.flags = [], []
        for i, (c, b) in enumerate(objects):
            b = np.asarray(b, np.float32).reshape(-1, 4)
            self.area.append(((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(np.float32) if area is None else np.asarray(area[i], np.float32).reshape(-1))
            crowded = np.zeros(len(b), np.uint8) if crowd is None else np.asarray(crowd[i]).astype(np.uint8).reshape(-1)
            self.flags.append(((self.gt[i][2] != 0) | ((crowded != 0) << 1)).astype(np.uint8))
            assert len(self.area[i]) == len(self.flags[i]) == len(b)
        self.scale = np.array([[w / cell_width, h / cell_height] for w, h in self.sizes], np.float32).reshape(-1, 2)
        self._keep = None

    def set_size(self, width, height):
        """The input size (one of ``input_sizes``) of the batches that follow: the images are resized to it, boxes and scales are restated
        in its cells.  Areas and flags are in source pixels and do not change."""
        pipe = self.pipe
        pipe.set_size(int(width), int(height))
        self.gt = gt_in_cells(self._objects, self.sizes, pipe.cell_width, pipe.cell_height, self._difficult)
        self.scale = np.array([[w / pipe.cell_width, h / pipe.cell_height] for w, h in self.sizes], np.float32).reshape(-1, 2)

    def __len__(self):
        return (len(self.sizes) + self.B - 1) // self.B

    def batch_gt(self, base, n_valid):
        """Host arrays (gt_class, gt_box, gt_difficult, gt_first [B+1]) of the images base .. base+n_valid-1, padded to B images."""
        cls, box, dif = [], [], []
        first = [0]
        for i in range(base, base + n_valid):
            c, b, d = self.gt[i]
            cls.append(c)
            box.append(b)
            dif.append(d)
            first.append(first[-1] + len(c))
        first += [first[-1]] * (self.B - n_valid)
        return (np.concatenate(cls).astype(np.int32), np.concatenate(box).astype(np.float32).reshape(-1, 4), np.concatenate(dif).astype(np.uint8),
                np.asarray(first, np.int32))

    def batch_gt_coco(self, base, n_valid):
        """Host arrays (gt_class, gt_box, gt_area, gt_flags, gt_first [B+1], scale [B,2]) of the same images; the padding's scale is 1."""
        cls, box, _, first = self.batch_gt(base, n_valid)
        scale = np.ones((self.B, 2), np.float32)
        scale[:n_valid] = self.scale[base:base + n_valid]
        return (cls, box, np.concatenate(self.area[base:base + n_valid]).astype(np.float32), np.concatenate(self.flags[base:base + n_valid]).astype(np.uint8),
                first, scale)

    def __iter__(self):
        return self.batches('voc')

    def batches(self, protocol='voc'):
        for base in range(0, len(self.sizes), self.B):
            n_valid = min(self.B, len(self.sizes) - base)
            images, gt = self.batch(base, n_valid, protocol)
            yield images, gt, base, n_valid

    def batch(self, base, n_valid, protocol='voc', flip=False, with_gt=True):
        """The images base .. base+n_valid-1 at the current size (padded to B) and their ground truth: one resize launch into the shared
        batch buffer.  ``flip`` sets the resize kernel's mirror flag (a test-time augmentation view: no extra launch, no copy); the ground truth
        is never mirrored.  ``with_gt`` False skips the ground truth's upload (-> None)."""
        pipe = self.pipe
        arr = pipe.assemble(list(range(base, base + n_valid)) + [0] * (self.B - n_valid))[0]
        assert all(a.flags == 0 and (a.crop_x, a.crop_y, a.crop_w, a.crop_h) == (0, 0, a.src_w, a.src_h) for a in arr)
        if flip:
            for a in arr:
                a.flags = AUGMENT_FLIP
        params = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
        ops.augment_images(pipe.src, params, pipe.ws, pipe.out, self.B, pipe.H, pipe.W, False)
        if not with_gt:
            gt = None
        elif protocol == 'coco':
            gt = device_gt_coco(*self.batch_gt_coco(base, n_valid))
        else:
            gt = tuple(device_gt(*self.batch_gt(base, n_valid)))
        self._keep = (params, gt)            # alive until the next batch (asynchronous kernels)
        return pipe.out, gt


def gt_in_cells(objects, sizes, cell_width, cell_height, difficult=None):
    """Per image (classes int32 [K], boxes f32 [K,4] in cell units, difficult uint8 [K]): pixel boxes times cells / image size, in
    float32 (the inverse of detect.py:49's scale)."""
    out = []
    for i, ((c, b), (w, h)) in enumerate(zip(objects, sizes)):
        c = np.asarray(c, np.int32).reshape(-1)
        scale = np.array([cell_width / w, cell_height / h] * 2, np.float32)
        b = (np.asarray(b, np.float32).reshape(-1, 4) * scale).astype(np.float32)
        d = np.zeros(len(c), np.uint8) if difficult is None else np.asarray(difficult[i]).astype(np.uint8).reshape(-1)
        assert len(b) == len(c) == len(d)
        out.append((c, b, d))
    return out


def device_gt(cls, box, dif, first, device='cuda'):
    """Host ground truth arrays -> device tensors, each with at least one element (the C ABI takes no null pointer)."""
    if len(cls) == 0:
        cls, box, dif = np.zeros(1, np.int32), np.zeros((1, 4), np.float32), np.zeros(1, np.uint8)
    return (torch.from_numpy(np.ascontiguousarray(cls, np.int32)).to(device), torch.from_numpy(np.ascontiguousarray(box, np.float32)).to(device),
            torch.from_numpy(np.ascontiguousarray(dif, np.uint8)).to(device), torch.from_numpy(np.ascontiguousarray(first, np.int32)).to(device))


def device_gt_coco(cls, box, area, flags, first, scale, device='cuda'):
    """Host ground truth arrays of the COCO protocol -> device tensors, each with at least one element."""
    if len(cls) == 0:
        area, flags = np.zeros(1, np.float32), np.zeros(1, np.uint8)
    c, b, f, o = device_gt(cls, box, flags, first, device)
    return (c, b, torch.from_numpy(np.ascontiguousarray(area, np.float32)).to(device), f, o, torch.from_numpy(np.ascontiguousarray(scale, np.float32)).to(device))


def records_per_image(N, C, mode, protocol='voc', fused=False, max_dets=100):
    """The most records one image can append: what ``evaluate`` sizes the record buffer by (times the number of images; the collect
    entries take at most 2^31 - 1 records).  N boxes of C classes: mode 'detect' one per box, mode 'all' one per (box, class) -- under the
    COCO protocol at most ``max_dets`` per class.  ``fused``: the N rows come from a test-time augmentation's fusion, where a row IS one
    (box, class) with a single score, so N rows are N records in either mode."""
    if fused:
        return min(N, max_dets * C) if protocol == 'coco' else N
    if protocol == 'coco':
        return min(N, max_dets) * C if mode == 'all' else N
    return N * (C if mode == 'all' else 1)


def evaluate(builder, session, data, mode='detect', threshold=0.005, threshold_iou=0.45, iou=0.5, preprocess_mode=0, max_records=None,
             evaluator=None, on_batch=None, protocol='voc', nms='hard', sigma=0.5, tta=None, fuse_iou=0.55, max_per_class=1024):
    """Runs ``session`` (a DetectSession whose batch equals data.B) over ``data`` (an EvalData) and returns Evaluator.result().
    threshold / threshold_iou go to detect() (score threshold and the NMS overlap), iou is the matching threshold.  on_batch(session, gt,
    image_base, n_valid), if given, is called after every detect (tests download the batch there).  protocol 'coco' scores with a
    CocoEvaluator instead (``iou`` is unused: its thresholds are the evaluator's table) and returns CocoEvaluator.result().  nms / sigma
    choose the suppression of detect(): 'hard' (the reference's), or Soft-NMS 'linear' / 'gaussian'.

    tta: the views (width, height, flip) the session was built with (``DetectSession(tta=...)``; ``data`` must have been built with their
    sizes as ``input_sizes``): every batch is run at each view -- assembled, run, suppressed and gathered before the next is assembled, since
    the batch buffer is shared -- and the views' boxes are fused by Weighted Boxes Fusion at the overlap ``fuse_iou`` (at most ``max_per_class``
    fused boxes per image and class).  The evaluator then sees the fused boxes: N = the session's ``tta_R`` rows in base-grid cells, one row per
    (fused box, class), so mode 'detect' and mode 'all' count the same detections.  The overflow flags are read once, after the last batch
    (``session.tta_check``): the loop does not synchronise.  on_batch sees the session after the fusion."""
    assert session.B == data.B, 'the session runs batches of %d, the data yields %d' % (session.B, data.B)
    if protocol not in ('voc', 'coco'):
        raise ValueError("protocol must be 'voc' or 'coco', not %r" % (protocol,))
    if tta:
        tta = [(int(w), int(h), bool(f)) for w, h, f in tta]
        if getattr(session, 'tta', None) != tta:
            raise ValueError('tta: the session was not built with these views (DetectSession(tta=...))')
    n = len(data.sizes)
    per_image = records_per_image(session.tta_R if tta else session.N, session.C, mode, protocol, fused=bool(tta))
    if evaluator is None and protocol == 'coco':
        evaluator = CocoEvaluator(session.C, max_records or n * per_image, mode=mode, threshold=threshold)
    if evaluator is None:
        evaluator = Evaluator(session.C, max_records or n * per_image, mode=mode, threshold=threshold, iou_threshold=iou)
    if tta:
        data.set_size(*tta[0][:2])                        # the ground truth in base-grid cells, once
        session.tta_begin()
        for base in range(0, n, data.B):
            n_valid = min(data.B, n - base)
            gt = None
            for v, (w, h, flip) in enumerate(tta):
                data.pipe.set_size(w, h)                   # (the images' size only: the ground truth stays in the base grid)
                images, g = data.batch(base, n_valid, protocol, flip=flip, with_gt=v == 0)
                gt = g if v == 0 else gt
                session.tta_add(images, (w, h, flip), threshold, threshold_iou, preprocess_mode, nms=nms, sigma=sigma)
            conf, xy_min, xy_max, _ = session.tta_fuse(threshold, fuse_iou, max_per_class=max_per_class)
            evaluator.add(conf, xy_min, xy_max, *gt, image_base=base, n_valid=n_valid)
            if on_batch is not None:
                on_batch(session, gt, base, n_valid)
        data.pipe.set_size(*tta[0][:2])
        session.tta_check()
        return evaluator.result()
    for images, gt, base, n_valid in data.batches(protocol):
        conf, xy_min, xy_max, _ = session.detect(images, threshold, threshold_iou, preprocess_mode, nms=nms, sigma=sigma)
        evaluator.add(conf, xy_min, xy_max, *gt, image_base=base, n_valid=n_valid)
        if on_batch is not None:
            on_batch(session, gt, base, n_valid)
    return evaluator.result()


def synthetic_dataset(n, classes, seed=0, max_objects=4):
    """Seeded random images of mixed sizes with random boxes: (images, objects, difficult) for EvalData."""
    rng = np.random.RandomState(seed)
    images, objects, difficult = [], [], []
    for _ in range(n):
        h, w = int(rng.randint(96, 320)), int(rng.randint(96, 320))
        images.append(rng.randint(0, 256, (h, w, 3)).astype(np.uint8))
        k = int(rng.randint(0, max_objects + 1))
        x0, y0 = rng.uniform(0, 0.7 * w, k), rng.uniform(0, 0.7 * h, k)
        x1, y1 = x0 + rng.uniform(0.1 * w, 0.3 * w, k), y0 + rng.uniform(0.1 * h, 0.3 * h, k)
        objects.append((rng.randint(0, classes, k).astype(np.int32), np.stack([x0, y0, x1, y1], 1).astype(np.float32).reshape(-1, 4)))
        difficult.append((rng.uniform(size=k) < 0.15).astype(np.uint8))
    return images, objects, difficult


def load_npz(path, coco=False):
    """The raw-object layout train.py accepts (images, objects_class, objects_coord, objects_first) plus an optional
    objects_difficult (default: all zero) -> (images, objects, difficult).  coco=True also reads the optional objects_crowd (default:
    all zero) and objects_area (source pixels squared; default None: EvalData takes the box area) and returns (images, objects,
    difficult, crowd, area)."""
    z = np.load(path, allow_pickle=True)
    images = list(z['images'])
    first = z['objects_first']
    cls, coord = z['objects_class'], z['objects_coord']
    per_image = lambda a, dtype: [np.asarray(a[first[i]:first[i + 1]], dtype) for i in range(len(images))]
    dif = z['objects_difficult'] if 'objects_difficult' in z.files else np.zeros(len(cls), np.uint8)
    objects = [(cls[first[i]:first[i + 1]], coord[first[i]:first[i + 1]]) for i in range(len(images))]
    difficult = per_image(dif, np.uint8)
    if not coco:
        return images, objects, difficult
    crowd = per_image(z['objects_crowd'] if 'objects_crowd' in z.files else np.zeros(len(cls), np.uint8), np.uint8)
    area = per_image(z['objects_area'], np.float32) if 'objects_area' in z.files else None
    return images, objects, difficult, crowd, area
