"""On-device evaluation of a detector: PASCAL VOC average precision (new work: the reference has no evaluator).

``Evaluator`` scores what a ``DetectSession`` leaves on the device after ``detect()``: ``add`` matches one batch against its ground
truth and appends (score, class, TP / FP / ignored, image, box) records to a buffer in HBM without synchronising, ``result`` sorts the
records per class on the device, integrates both VOC metrics there and downloads one small block.  ``EvalData`` walks a dataset held
in HBM in order, ``evaluate`` ties the two to a session.  The rules (include/yolo2_hip.h, section "evaluation") are the VOC devkit's:
COCO's protocol (101 recall points, IoU 0.5:0.95, area ranges, best unmatched candidate) is not implemented.
"""
import math

import numpy as np
import torch

from . import ops
from ._lib import HipKernelError, query
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


class EvalData(object):
    """A sequential, unshuffled, unaugmented walk over a dataset held in HBM.

    images: list of uint8 [h, w, 3] arrays (any sizes); objects: list of (classes int [K], boxes float [K,4] in pixels of the image:
    xmin, ymin, xmax, ymax); difficult: list of [K] flags or None (all zero: the reference's dataset cache has no such field).
    Iterating yields (image batch f32 [B,H,W,3] 0..255, (gt_class, gt_box, gt_difficult, gt_first) device tensors with the boxes in
    CELL units, image_base, n_valid).  The last batch is padded to B with copies of the dataset's first image that own no ground
    truth; n_valid says how many images count.

    The resize is the device's TF-style bilinear one (yolo2_augment_images with the full-image crop and no flags), the one training
    sees.  It is NOT the PIL resize detect.py applies to a file, so scores can differ slightly from what detect.py prints."""

    def __init__(self, images, objects, batch, width, height, cell_width, cell_height, difficult=None):
        # the training pipeline with every augmentation disabled: its draw() then yields the full-image crop and no flags
        self.pipe = DeviceInputPipeline(images, objects, batch, width, height, None, cell_width, cell_height, config=AugmentConfig(None))
        self.B, self.sizes = batch, self.pipe.sizes
        self.gt = gt_in_cells(objects, self.sizes, cell_width, cell_height, difficult)
        self._keep = None

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

    def __iter__(self):
        for base in range(0, len(self.sizes), self.B):
            n_valid = min(self.B, len(self.sizes) - base)
            pipe = self.pipe
            arr = pipe.assemble(list(range(base, base + n_valid)) + [0] * (self.B - n_valid))[0]
            assert all(a.flags == 0 and (a.crop_x, a.crop_y, a.crop_w, a.crop_h) == (0, 0, a.src_w, a.src_h) for a in arr)
            params = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
            ops.augment_images(pipe.src, params, pipe.ws, pipe.out, self.B, pipe.H, pipe.W, False)
            gt = tuple(device_gt(*self.batch_gt(base, n_valid)))
            self._keep = (params, gt)            # alive until the next batch (asynchronous kernels)
            yield pipe.out, gt, base, n_valid


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


def evaluate(builder, session, data, mode='detect', threshold=0.005, threshold_iou=0.45, iou=0.5, preprocess_mode=0, max_records=None,
             evaluator=None, on_batch=None):
    """Runs ``session`` (a DetectSession whose batch equals data.B) over ``data`` (an EvalData) and returns Evaluator.result().
    threshold / threshold_iou go to detect() (score threshold and the NMS overlap), iou is the matching threshold.  on_batch(session, gt,
    image_base, n_valid), if given, is called after every detect (tests download the batch there)."""
    assert session.B == data.B, 'the session runs batches of %d, the data yields %d' % (session.B, data.B)
    n = len(data.sizes)
    if evaluator is None:
        per_image = session.N * (session.C if mode == 'all' else 1)
        evaluator = Evaluator(session.C, max_records or n * per_image, mode=mode, threshold=threshold, iou_threshold=iou)
    for images, gt, base, n_valid in data:
        conf, xy_min, xy_max, _ = session.detect(images, threshold, threshold_iou, preprocess_mode)
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


def load_npz(path):
    """The raw-object layout train.py accepts (images, objects_class, objects_coord, objects_first) plus an optional
    objects_difficult (default: all zero) -> (images, objects, difficult)."""
    z = np.load(path, allow_pickle=True)
    images = list(z['images'])
    first = z['objects_first']
    cls, coord = z['objects_class'], z['objects_coord']
    dif = z['objects_difficult'] if 'objects_difficult' in z.files else np.zeros(len(cls), np.uint8)
    objects = [(cls[first[i]:first[i + 1]], coord[first[i]:first[i + 1]]) for i in range(len(images))]
    difficult = [np.asarray(dif[first[i]:first[i + 1]], np.uint8) for i in range(len(images))]
    return images, objects, difficult
