"""Dimension clusters: the anchors of a dataset, fitted on the device (new work; the reference lists "Dimension cluster" as an unchecked
roadmap item, README.md:88, and only reads the result: model/yolo2/__init__.py:106).  YOLO9000, section 2 "Dimension Clusters": k-means
over the ground truth boxes' (w, h) with distance 1 - IoU, k chosen from a sweep.  The semantics (operation order, fixed-point sums,
fixed point detection) are those of include/yolo2_hip.h, section "dimension clusters"; tests/anchors_ref.py restates them in NumPy.

Host side: ``boxes_in_cells`` and the readers turn a dataset into f32 [N][2] boxes in grid-cell units, ``write_anchors`` writes the TSV
``utils.read_anchors`` reads.  Device side: ``DimensionClusters`` uploads the boxes once and runs many (k, restart) jobs per launch."""
import os

import numpy as np

MIN_VALUE = 2.0 ** -12       # valid box extents, in cells: MIN_VALUE <= v < MAX_VALUE (the fixed-point sums of the kernels rely on it)
MAX_VALUE = 2.0 ** 12
MAX_K = 32                   # YOLO2_ANCHOR_MAX_K
MAX_JOBS = 65535             # YOLO2_ANCHOR_MAX_JOBS
MAX_BOXES = (1 << 27) - 1    # YOLO2_ANCHOR_MAX_BOXES


# ---------------------------------------------------------------- host: boxes of a dataset
def boxes_in_cells(objects, sizes, cells_x, cells_y):
    """objects: per image (classes, coords [K,4] = xmin, ymin, xmax, ymax in pixels); sizes: per image (width, height) in pixels.
    Returns f32 [N][2] = (w, h) of every box in grid-cell units, the unit of config/yolo2/anchors/*.tsv: (xmax - xmin) / width * cells_x
    and (ymax - ymin) / height * cells_y, evaluated in f64 and rounded to f32 once.  Nothing is dropped: a box of non-positive or
    non-finite extent raises ValueError, and so does an image of non-positive size."""
    out = []
    for i, ((_, coords), (width, height)) in enumerate(zip(objects, sizes)):
        b = np.asarray(coords, np.float32).reshape(-1, 4).astype(np.float64)
        if not (width > 0 and height > 0):
            raise ValueError('image %d: size %r x %r' % (i, width, height))
        wh = np.stack([(b[:, 2] - b[:, 0]) / float(width) * cells_x, (b[:, 3] - b[:, 1]) / float(height) * cells_y], 1)
        bad = ~(np.isfinite(wh).all(1) & (wh > 0).all(1))
        if bad.any():
            raise ValueError('image %d, box %d: extent %r is not positive' % (i, int(np.argmax(bad)), tuple(wh[np.argmax(bad)])))
        out.append(wh.astype(np.float32))
    if not out:
        return np.zeros((0, 2), np.float32)
    return np.ascontiguousarray(np.concatenate(out, 0), np.float32)


def cache_objects(paths):
    """(objects, sizes) of the reference's TFRecord cache files: the records carry the image shape and the boxes, so no image is opened."""
    from .utils import tfrecord
    objects, sizes = [], []
    for _, shape, cls, coord in tfrecord.read_cache(paths):
        objects.append((cls, coord))
        sizes.append((shape[1], shape[0]))          # imageshape is (height, width, channels)
    return objects, sizes


def npz_objects(path):
    """(objects, sizes) of a .npz in the raw-object layout evaluate.load_npz documents (images, objects_class, objects_coord,
    objects_first); only the images' shapes are used."""
    z = np.load(path, allow_pickle=True)
    first, cls, coord = z['objects_first'], z['objects_class'], z['objects_coord']
    images = z['images']
    objects = [(cls[first[i]:first[i + 1]], coord[first[i]:first[i + 1]]) for i in range(len(images))]
    sizes = [(np.shape(im)[1], np.shape(im)[0]) for im in images]
    return objects, sizes


def synthetic_boxes(n, cells_x, cells_y, seed=0):
    """n seeded log-normal boxes in cell units (median a fifth of the grid, sigma 0.7 in w and in the aspect ratio), clipped to the grid."""
    rng = np.random.RandomState(seed)
    w = np.exp(rng.normal(np.log(cells_x / 5.0), 0.7, n))
    h = w * np.exp(rng.normal(np.log(float(cells_y) / cells_x), 0.7, n))
    return np.ascontiguousarray(np.stack([np.clip(w, 0.05, cells_x), np.clip(h, 0.05, cells_y)], 1), np.float32)


def read_boxes(data, cells_x, cells_y, cache_paths=None, n=None, seed=0):
    """Boxes of one of the three sources the command line tools know: 'cache' (``cache_paths``: TFRecord cache files), 'synthetic'
    (``n`` boxes from ``seed``) or the path of a .npz file."""
    if data == 'synthetic':
        return synthetic_boxes(n, cells_x, cells_y, seed)
    objects, sizes = cache_objects(cache_paths) if data == 'cache' else npz_objects(os.path.expanduser(os.path.expandvars(data)))
    return boxes_in_cells(objects, sizes, cells_x, cells_y)


def validate_boxes(boxes):
    """f32 [N][2], contiguous; ValueError unless 1 <= N <= MAX_BOXES and every value is finite with MIN_VALUE <= v < MAX_VALUE."""
    a = np.asarray(boxes)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError('boxes must be [N][2] (w, h), not %r' % (a.shape,))
    if not 1 <= len(a) <= MAX_BOXES:
        raise ValueError('%d boxes: need 1 .. %d' % (len(a), MAX_BOXES))
    a = np.ascontiguousarray(a, np.float32)
    if not (np.isfinite(a).all() and (a >= MIN_VALUE).all() and (a < MAX_VALUE).all()):
        raise ValueError('box extents must be finite with 2**-12 <= v < 2**12 (cell units)')
    return a


def write_anchors(path, anchors):
    """The reference's anchor TSV (`w<TAB>h` header, one tab-separated row per anchor); utils.read_anchors returns the same f32 values
    (repr of a float32 is the shortest text that reads back to it)."""
    a = np.asarray(anchors, np.float32).reshape(-1, 2)

    def text(v):
        t = np.format_float_positional(v, unique=True, trim='0')
        return t if np.float32(float(t)) == v else repr(float(v))          # (read back through f64: keep the exact value if that ever differs)
    with open(os.path.expanduser(os.path.expandvars(path)), 'w') as f:
        f.write('w\th\n')
        for w, h in a:
            f.write('%s\t%s\n' % (text(w), text(h)))


def job_table(ks, restarts):
    """The job order of a sweep: for every k in the order given, restarts 0 .. restarts - 1.  Returns (job_k, job_restart) int32."""
    ks = [int(k) for k in ks]
    return (np.repeat(np.asarray(ks, np.int32), restarts), np.tile(np.arange(restarts, dtype=np.int32), len(ks)))


def initial_indices(n, job_k, seed):
    """Initialisation, the host's: ONE numpy.random.RandomState(seed) serves the jobs in job order; a job draws rng.randint(0, n) until it
    holds k distinct box indices, kept in order of first appearance.  (k distinct indices without replacement, at a cost that does not
    grow with n.)  k > n raises ValueError."""
    rng = np.random.RandomState(seed)
    out = []
    for k in job_k:
        k = int(k)
        if k > n:
            raise ValueError('k = %d centroids from %d boxes' % (k, n))
        idx = []
        seen = set()
        while len(idx) < k:
            i = int(rng.randint(0, n))
            if i not in seen:
                seen.add(i)
                idx.append(i)
        out.append(np.asarray(idx, np.int64))
    return out


def sort_by_area(anchors, counts=None):
    """Anchors sorted by area ascending (stable; the f64 product of the f32 values is exact), counts permuted alike."""
    a = np.asarray(anchors, np.float32).reshape(-1, 2)
    order = np.argsort(a[:, 0].astype(np.float64) * a[:, 1].astype(np.float64), kind='stable')
    return (a[order], None if counts is None else np.asarray(counts)[order])


# ---------------------------------------------------------------- device
class DimensionClusters(object):
    """Validates the boxes and uploads them once; ``fit`` and ``score`` then run on the device."""

    def __init__(self, boxes, device=None):
        import torch
        self.boxes_host = validate_boxes(boxes)
        self.n = len(self.boxes_host)
        self.device = torch.device('cuda' if device is None else device)
        self.boxes = torch.from_numpy(self.boxes_host).to(self.device)

    def run_jobs(self, job_k, centroids, max_iter=500, check_every=16, assignments=()):
        """The job table as it runs on the device.  job_k [J] int, centroids [J][kmax][2] f32 (slots at and past job_k[j] are carried
        along untouched).  Runs assign + update pairs until every job is at its fixed point or ``max_iter`` updates have been applied,
        looking at the device only every ``check_every`` iterations (a frozen job is left alone, so the answer does not depend on it),
        then one score pass.  Returns a dict of host arrays: centroids, iterations [J], converged [J] bool, avg_iou [J] f64, counts
        [J][kmax] int64 (-1 at and past job_k[j]), and assignments {j: uint8 [N]} for the jobs named in ``assignments``."""
        import torch

        from . import ops
        job_k = np.ascontiguousarray(job_k, np.int32).reshape(-1)
        cen = np.ascontiguousarray(centroids, np.float32)
        J = len(job_k)
        if cen.ndim != 3 or cen.shape[0] != J or cen.shape[2] != 2:
            raise ValueError('centroids must be [jobs][kmax][2], not %r for %d jobs' % (cen.shape, J))
        kmax = cen.shape[1]
        if not (1 <= J <= MAX_JOBS and 1 <= kmax <= MAX_K and (job_k >= 1).all() and (job_k <= kmax).all()):
            raise ValueError('need 1 <= jobs <= %d and 1 <= k <= kmax <= %d' % (MAX_JOBS, MAX_K))
        if max_iter < 0 or check_every < 1:
            raise ValueError('max_iter >= 0 and check_every >= 1')
        for j in range(J):
            validate_boxes(cen[j, :job_k[j]])          # a centroid is a box: same range
        with torch.cuda.device(self.device):
            dev = self.device
            d_cen = torch.from_numpy(cen).to(dev)
            d_k = torch.from_numpy(job_k).to(dev)
            words = 3 * kmax + 1
            assert ops.workspace_bytes('anchor', J, kmax) == 8 * J * words
            ws = torch.zeros(J * words, dtype=torch.int64, device=dev)          # zeroed once: every update / score pass clears what it read
            done = torch.zeros(J, dtype=torch.int32, device=dev)
            iterations = torch.zeros(J, dtype=torch.int32, device=dev)
            counts = torch.full((J, kmax), -1, dtype=torch.int64, device=dev)
            avg = torch.zeros(J, dtype=torch.float64, device=dev)
            for it in range(1, max_iter + 1):
                ops.anchor_assign(self.boxes, self.n, d_cen, d_k, J, kmax, ws, done=done)
                ops.anchor_update(d_cen, d_k, J, kmax, ws, self.n, done=done, iterations=iterations)
                if it % check_every == 0 and int(done.sum().item()) == J:          # the only synchronisation of the loop
                    break
            ops.anchor_assign(self.boxes, self.n, d_cen, d_k, J, kmax, ws)
            ops.anchor_update(None, d_k, J, kmax, ws, self.n, counts=counts, avg_iou=avg)
            out_assign = {}
            for j in assignments:
                a = torch.empty(self.n, dtype=torch.uint8, device=dev)
                scratch = torch.empty(1, dtype=torch.float64, device=dev)
                ops.anchor_assign(self.boxes, self.n, d_cen[j:j + 1], d_k[j:j + 1], 1, kmax, ws, assignment=a)
                ops.anchor_update(None, d_k[j:j + 1], 1, kmax, ws, self.n, avg_iou=scratch)
                out_assign[int(j)] = a.cpu().numpy()
            return dict(centroids=d_cen.cpu().numpy(), iterations=iterations.cpu().numpy(), converged=done.cpu().numpy().astype(bool),
                        avg_iou=avg.cpu().numpy(), counts=counts.cpu().numpy(), assignments=out_assign, job_k=job_k)

    def fit(self, ks, restarts=16, max_iter=500, seed=0, check_every=16):
        """k-means for every k of ``ks`` x ``restarts`` random initialisations, all in the same launches.  Jobs are ordered as
        ``job_table`` says and initialised as ``initial_indices`` says.  Returns {k: dict} with the best restart's (highest avg_iou,
        of equal ones the first) ``anchors`` [k][2] sorted by area ascending, its ``avg_iou``, ``counts`` (in anchor order),
        ``iterations``, ``converged`` and ``restart``, and every restart's ``restart_avg_iou``."""
        ks = [int(k) for k in ks]
        if not ks or restarts < 1 or len(set(ks)) != len(ks) or min(ks) < 1 or max(ks) > MAX_K:
            raise ValueError('ks: distinct values in 1 .. %d; restarts >= 1' % MAX_K)
        job_k, _ = job_table(ks, restarts)
        kmax = max(ks)
        cen = np.zeros((len(job_k), kmax, 2), np.float32)
        for j, idx in enumerate(initial_indices(self.n, job_k, seed)):
            cen[j, :len(idx)] = self.boxes_host[idx]
        r = self.run_jobs(job_k, cen, max_iter=max_iter, check_every=check_every)
        out = {}
        for i, k in enumerate(ks):
            sl = slice(i * restarts, (i + 1) * restarts)
            best = int(np.argmax(r['avg_iou'][sl]))
            j = i * restarts + best
            anchors, counts = sort_by_area(r['centroids'][j, :k], r['counts'][j, :k])
            out[k] = dict(anchors=anchors, avg_iou=float(r['avg_iou'][j]), counts=counts, iterations=int(r['iterations'][j]),
                          converged=bool(r['converged'][j]), restart=best, restart_avg_iou=[float(v) for v in r['avg_iou'][sl]])
        self.last_jobs = r
        return out

    def score(self, anchors, assignment=False):
        """Average IoU of every box with its best anchor and the boxes per anchor: (avg_iou, counts [k]), plus the uint8 [N] assignment
        when asked.  ``DimensionClusters(boxes).score(utils.read_anchors('config/yolo2/anchors/voc.tsv'))`` says how well the shipped
        anchors fit a dataset."""
        a = np.ascontiguousarray(anchors, np.float32).reshape(-1, 2)
        r = self.run_jobs([len(a)], a[None], max_iter=0, assignments=(0,) if assignment else ())
        res = (float(r['avg_iou'][0]), r['counts'][0, :len(a)])
        return res + (r['assignments'][0],) if assignment else res
