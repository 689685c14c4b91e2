"""COCO key-point annotation files -> what the training entries take: poses and ignore masks.

The reference reads annotations with `pycocotools` (coco_data_loader.py:270-332) and the ignore masks from PNG files a separate program
writes first (gen_ignore_mask.py:23-37, `annToMask` per annotation).  This module reads the annotation file with `json` alone and states
the masks as a contract of its own, in NumPy, below; `pmx_coco_masks` (csrc/pmx_masks.hip) computes the same bytes on the device per
batch, so the `ignore_mask_*2017` directories are no prerequisite any more.

  CocoKeypoints                       the annotation file: image ids, annotations per image, the reference's validity filter
  parse_annotations                   annotations -> (n, 18, 3) int32 poses (parse_coco_annotation)
  mask_classes / mask_parts           per annotation its class (keep / miss / crowd) and its segmentation as polygon / run-length parts
  polygon_mask / rle_mask / masks_numpy   THE MASK CONTRACT (host NumPy; the oracle of the device entry, like the NumPy drawing functions)
  batches                             annotation file + image directory -> the (imgs, poses, masks) triples of train_loop / train_step
  detections / ground_truths          what the key-point evaluation sees of a detector's output and of an image's annotations
  oks_matrix / evaluate_image         THE EVALUATION CONTRACT per image (host NumPy; the oracle of pmx_coco_eval, csrc/pmx_eval.hip)
  accumulate / summarize              precision / recall over a data set and the ten AP / AR numbers (host only)
  results                             detections in the COCO results format, for the official tool elsewhere
  evaluate                            annotation file + image directory + detector -> AP / AR, the per-image part on the device

The mask contract restates `annToMask` of the library's C part (rleFrPoly + rleMerge + rleDecode) from its published source.  The library
is not a dependency and the restatement has not been compared with it bit for bit: that pin is open.
The evaluation contract restates `COCOeval` with iouType = 'keypoints' (and `loadRes` for the detections' areas) from the same published
source, under the same terms: no dependency, and its pin against the real library is open too -- `results` writes the detections in the
format the official tool reads, so the same detections can be scored there.
"""
import json
import os

import numpy as np

from .entity import JointType, params

KEEP, MISS, CROWD = 0, 1, 2          # mask_classes: how gen_masks treats an annotation
POLYGON, RLE = 0, 1                  # kinds of a part (pmx_mask_part.kind)
COORD_LIMIT = 65536.0                # polygon coordinates lie within +-COORD_LIMIT (5 * x + .5 then fits a C int with room to spare)


class CocoKeypoints(object):
    """One COCO annotation file (a path, or the dictionary `json.load` gives).  mode: 'train' | 'val' | 'eval', as CocoDataLoader's."""

    def __init__(self, annotation_file_or_dict, mode='train'):
        if mode not in ('train', 'val', 'eval'):
            raise ValueError("CocoKeypoints: mode must be 'train', 'val' or 'eval'")
        self.mode = mode
        data = annotation_file_or_dict
        if not isinstance(data, dict):
            with open(data) as f:
                data = json.load(f)
        self.images = {im['id']: im for im in data.get('images', [])}
        self._anns = {}
        for ann in data.get('annotations', []):          # file order within an image = getAnnIds(imgIds=[id], iscrowd=None)
            self._anns.setdefault(ann['image_id'], []).append(ann)
        # sorted(getImgIds(catIds=getCatIds())): the images with at least one annotation (a key-point file has the one category 'person')
        self.img_ids = sorted(self._anns)

    def __len__(self):
        return len(self.img_ids)

    def annotations(self, img_id):
        """every annotation of the image, in file order (what gen_ignore_mask.py rasterises)"""
        return list(self._anns.get(img_id, []))

    def valid_annotations(self, img_id):
        """the annotations get_img_annotation keeps (coco_data_loader.py:286): enough key points and large enough; None if none is left"""
        keep = [a for a in self._anns.get(img_id, [])
                if a['num_keypoints'] >= params['min_keypoints'] and a['area'] > params['min_area']]
        return keep or None

    def example_annotations(self, img_id):
        """what get_img_annotation returns as annotations: every one in mode 'eval' (:307-308), else the valid ones or None"""
        return self.annotations(img_id) if self.mode == 'eval' else self.valid_annotations(img_id)

    def size(self, img_id):
        im = self.images[img_id]
        return int(im['height']), int(im['width'])

    def file_name(self, img_id):
        return self.images[img_id]['file_name']


def parse_annotations(annotations):
    """parse_coco_annotation (coco_data_loader.py:311-332): (n, 18, 3) int32 rows (x, y, v); the neck is the truncated mean of the
    shoulders, v = 2, where both shoulders are labelled."""
    poses = np.zeros((len(annotations), len(JointType), 3), dtype=np.int32)
    L, R, N = int(JointType.LeftShoulder), int(JointType.RightShoulder), int(JointType.Neck)
    for pose, ann in zip(poses, annotations):
        ann_pose = np.array(ann['keypoints']).reshape(-1, 3)
        for i, joint_index in enumerate(params['coco_joint_indices']):
            pose[joint_index] = ann_pose[i]
        if pose[L][2] > 0 and pose[R][2] > 0:
            pose[N][0] = int((int(pose[L][0]) + int(pose[R][0])) / 2)
            pose[N][1] = int((int(pose[L][1]) + int(pose[R][1])) / 2)
            pose[N][2] = 2
    return poses


def mask_classes(annotations):
    """One class per annotation, as gen_masks branches (gen_ignore_mask.py:28-36): CROWD (iscrowd == 1), MISS (too few key points or too
    small), else KEEP."""
    out = np.zeros(len(annotations), dtype=np.int32)
    for i, a in enumerate(annotations):
        if a['iscrowd'] == 1:
            out[i] = CROWD
        elif a['num_keypoints'] < params['min_keypoints'] or a['area'] <= params['min_area']:
            out[i] = MISS
    return out


def mask_parts(annotations, h, w):
    """The segmentations of an image's annotations as a flat list of parts (kind, annotation index, class, data): a list of polygons gives
    one POLYGON part per polygon (data: the flat [x0, y0, x1, y1, ...] float64 array), a dictionary {'counts': [ints], 'size': [h, w]}
    one RLE part (data: the counts, uint32).  ValueError for: a compressed `counts` string; a polygon with fewer than 6 numbers or an odd
    count; coordinates that are not finite or outside +-65536; an RLE `size` that is not the image's; counts that do not sum to h * w.
    NOTE: the library reads a segmentation whose first polygon has exactly four numbers as a box; such a segmentation is refused here
    (fewer than 6 numbers), like every polygon of fewer than three vertices."""
    h, w = int(h), int(w)
    classes = mask_classes(annotations)
    parts = []
    for i, a in enumerate(annotations):
        seg = a['segmentation']
        if isinstance(seg, dict):
            counts = seg.get('counts')
            if isinstance(counts, (str, bytes)):
                raise ValueError('annotation %d: compressed run-length counts are not supported (uncompressed lists only)' % i)
            if [int(v) for v in seg.get('size', ())] != [h, w]:
                raise ValueError('annotation %d: run-length size %r, the image is %r' % (i, seg.get('size'), [h, w]))
            c = np.asarray(counts, dtype=np.int64).reshape(-1)
            if c.size and c.min() < 0 or int(c.sum()) != h * w:
                raise ValueError('annotation %d: run-length counts sum to %d, the image has %d pixels' % (i, int(c.sum()), h * w))
            parts.append((RLE, i, int(classes[i]), c.astype(np.uint32)))
        else:
            for poly in seg:
                xy = np.asarray(poly, dtype=np.float64).reshape(-1)
                if xy.size < 6 or xy.size % 2:
                    raise ValueError('annotation %d: a polygon of %d numbers (at least 6, an even count)' % (i, xy.size))
                if not np.all(np.isfinite(xy)) or np.abs(xy).max() > COORD_LIMIT:
                    raise ValueError('annotation %d: polygon coordinates must be finite and within +-%d' % (i, COORD_LIMIT))
                parts.append((POLYGON, i, int(classes[i]), xy))
    return parts


# ---- the mask contract ----------------------------------------------------------------------------------------------------------------
def polygon_crossings(xy, h, w):
    """Steps 1-3 of the contract for one polygon: the crossing points (xd, yd), int64 arrays in list order.  All arithmetic is that of C
    `double` and `int`; (int) truncates toward zero."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1)
    k = xy.size // 2
    # 1. scale: X = (int)(5 * x + .5), closed
    X = np.trunc(5 * xy[0::2] + .5).astype(np.int64)
    Y = np.trunc(5 * xy[1::2] + .5).astype(np.int64)
    X, Y = np.append(X, X[0]), np.append(Y, Y[0])
    # 2. trace every edge into a dense point list
    us, vs = [], []
    for j in range(k):
        xs, xe, ys, ye = int(X[j]), int(X[j + 1]), int(Y[j]), int(Y[j + 1])
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            d = np.arange(dx + 1, dtype=np.int64)
            t = dx - d if flip else d
            u = t + xs
            if dx == 0:          # a zero-length edge: its vertex once (the C code divides 0 by 0 here; v is Y, never a crossing of its own)
                v = np.full(1, ys, dtype=np.int64)
            else:
                s = np.float64(ye - ys) / np.float64(dx)
                v = np.trunc(ys + s * t + .5).astype(np.int64)
        else:
            d = np.arange(dy + 1, dtype=np.int64)
            t = dy - d if flip else d
            s = np.float64(xe - xs) / np.float64(dy)
            u = np.trunc(xs + s * t + .5).astype(np.int64)
            v = t + ys
        us.append(u)
        vs.append(v)
    u, v = np.concatenate(us), np.concatenate(vs)
    # 3. crossing points: consecutive pairs whose u differs
    p = np.nonzero(u[1:] != u[:-1])[0] + 1
    m = np.where(u[p] < u[p - 1], u[p], u[p] - 1).astype(np.float64)
    xd = (m + .5) / 5 - .5
    ok = (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
    yd = (np.minimum(v[p], v[p - 1]).astype(np.float64) + .5) / 5 - .5
    yd = np.ceil(np.clip(yd, 0, h))
    return xd[ok].astype(np.int64), yd[ok].astype(np.int64)


def polygon_mask(xy, h, w):
    """One polygon part -> (h, w) uint8 of 0 / 1.  Step 4: pixel (x, y) is 1 iff the number of crossing points of column x with yd <= y is
    odd; points with yd == h close a run at the column's end.  The count of every column is even (asserted), so columns are independent."""
    h, w = int(h), int(w)
    xd, yd = polygon_crossings(xy, h, w)
    cnt = np.zeros((w, h + 1), dtype=np.int64)
    np.add.at(cnt, (xd, yd), 1)
    if np.any(cnt.sum(axis=1) & 1):
        raise AssertionError('polygon_mask: a column with an odd number of crossing points')
    return np.ascontiguousarray((np.cumsum(cnt, axis=1)[:, :h] & 1).T.astype(np.uint8))


def rle_mask(counts, h, w):
    """One run-length part: runs of 0 and 1 in turn, starting with 0, over the column-major index x * h + y."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    if int(counts.sum()) != int(h) * int(w):
        raise ValueError('rle_mask: counts sum to %d, the image has %d pixels' % (int(counts.sum()), int(h) * int(w)))
    bits = np.repeat((np.arange(counts.size) & 1).astype(np.uint8), counts)
    return np.ascontiguousarray(bits.reshape(int(w), int(h)).T)


def masks_numpy(h, w, parts):
    """(mask_miss, mask_all) of one image, (h, w) uint8 of 0 / 1 each, from its parts (mask_parts) -- gen_masks (gen_ignore_mask.py:23-37).
    An annotation's mask is the union of its parts.  In file order, with `all` as it was before the annotation:
        crowd: miss |= mask & ~all;  miss: miss |= mask;  then in every case all |= mask.
    The reference writes the crowd case as `mask - intxn` on bool arrays (intxn = all & mask), which current NumPy refuses; under the NumPy
    it was written for that was XOR, and mask ^ (all & mask) is mask & ~all."""
    h, w = int(h), int(w)
    mask_all, mask_miss = np.zeros((h, w), bool), np.zeros((h, w), bool)
    i = 0
    parts = list(parts)
    while i < len(parts):
        ann, cls = parts[i][1], parts[i][2]
        mask = np.zeros((h, w), bool)
        while i < len(parts) and parts[i][1] == ann:
            kind, _, _, data = parts[i]
            mask |= (polygon_mask(data, h, w) if kind == POLYGON else rle_mask(data, h, w)).astype(bool)
            i += 1
        if cls == CROWD:
            mask_miss |= mask & ~mask_all
        elif cls == MISS:
            mask_miss |= mask
        mask_all |= mask
    return mask_miss.astype(np.uint8), mask_all.astype(np.uint8)


# ---- the way into training ------------------------------------------------------------------------------------------------------------
def batches(dataset, detector, image_dir, batch, insize=368, mode='train', rng=None):
    """One pass over `dataset` (a CocoKeypoints) in image-id order: yields (imgs (B, insize, insize, 3) uint8, poses per image (n, 18, 3)
    int32, masks (B, insize, insize) bool), B <= batch -- what train_loop, train_step and validation_loss take.  Images are read from
    `image_dir` (file names of the annotation file); an image without valid annotations is replaced by a random draw
    (`rng.randint(len(dataset))`, default np.random) until one has some, as get_example does (coco_data_loader.py:351-353).  The ignore
    masks are rasterised on the device from ALL annotations of an image (detector.ignore_masks(..., device=True)) and go to
    prepare_samples with the images as device tensors: no mask visits the host on the way."""
    import torch
    from .pose_detector import imread_bgr
    rng = np.random if rng is None else rng
    batch = int(batch)
    if batch < 1:
        raise ValueError('batches: batch = %d' % batch)
    dev = torch.device('cuda', detector._gpu)
    detector._grow(1, int(insize), int(insize))          # the engine that rasterises the masks is the one that prepares the samples
    for i in range(0, len(dataset), batch):
        imgs, poses, anns = [], [], []
        for img_id in dataset.img_ids[i:i + batch]:
            valid = dataset.valid_annotations(img_id)
            while valid is None:
                img_id = dataset.img_ids[rng.randint(len(dataset))]
                valid = dataset.valid_annotations(img_id)
            img = imread_bgr(os.path.join(image_dir, dataset.file_name(img_id)))
            imgs.append(torch.from_numpy(np.ascontiguousarray(img)).to(dev))
            poses.append(parse_annotations(valid))
            anns.append(dataset.annotations(img_id))
        masks = detector.ignore_masks(anns, [tuple(im.shape[:2]) for im in imgs], device=True)
        yield detector.prepare_samples(imgs, poses, masks, insize=insize, mode=mode)


# ---- the evaluation contract -----------------------------------------------------------------------------------------------------------
# COCOeval with iouType = 'keypoints' (computeOks, evaluateImg, accumulate, summarize; loadRes for the detections' areas), restated
# from the library's published source.  The constants are computed with the library's own expressions, in float64, once; the device
# entry gets these very doubles (eval_consts).
KP_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
KP_VARS = (KP_SIGMAS * 2) ** 2
KP_EPS = np.spacing(1)
IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = 20
AREA_RNGS = [[0, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LABELS = ('all', 'medium', 'large')
EVAL_MAX_GT = 512                    # PMX_EVAL_MAX_GT: ground truths of one image the device entry takes
SUMMARY_KEYS = ('AP', 'AP50', 'AP75', 'AP_medium', 'AP_large', 'AR', 'AR50', 'AR75', 'AR_medium', 'AR_large')


def detections(poses, scores):
    """The detections of one image as the evaluation sees them: {'keypoints' (n, 17, 3) float64, 'score' (n,), 'area' (n,)} from the
    (n, 18, 3) poses and the scores a detector returns.  COCO key point i is joint params['coco_joint_indices'][i] (the neck is
    dropped): (x, y, 1) where the joint was found (v != 0), else (0, 0, 0).  The score is the record's score, subsets[:, -2]: the sum of
    the person's peak and connection scores -- the number the detector itself ranks hypotheses by; the reference publishes no COCO score,
    and the evaluation only uses the order it gives.  area = (max x - min x) * (max y - min y) over all 17 points, zeros included, as
    loadRes computes it."""
    poses = np.asarray(poses, dtype=np.float64)
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    if poses.size == 0:
        poses = np.zeros((0, len(JointType), 3))
    if poses.ndim != 3 or poses.shape[1:] != (len(JointType), 3) or len(poses) != len(scores):
        raise ValueError('detections: poses (n, 18, 3) and n scores expected, got %r and %r' % (poses.shape, scores.shape))
    rows = poses[:, [int(j) for j in params['coco_joint_indices']], :]
    found = rows[:, :, 2] != 0
    kp = np.zeros((len(poses), 17, 3))
    kp[:, :, 0] = np.where(found, rows[:, :, 0], 0.0)
    kp[:, :, 1] = np.where(found, rows[:, :, 1], 0.0)
    kp[:, :, 2] = found
    if len(kp):
        area = (kp[:, :, 0].max(axis=1) - kp[:, :, 0].min(axis=1)) * (kp[:, :, 1].max(axis=1) - kp[:, :, 1].min(axis=1))
    else:
        area = np.zeros(0)
    return {'keypoints': kp, 'score': scores.copy(), 'area': area}


def ground_truths(annotations):
    """Every annotation of one image, in file order, as the evaluation sees it: {'keypoints' (G, 17, 3), 'area', 'bbox' (G, 4), 'iscrowd',
    'num_keypoints', 'ignore'}; ignore = iscrowd == 1 or num_keypoints == 0, num_keypoints taken from the field.  A dictionary this
    function made passes through."""
    if isinstance(annotations, dict):
        return annotations
    G = len(annotations)
    out = {'keypoints': np.zeros((G, 17, 3)), 'area': np.zeros(G), 'bbox': np.zeros((G, 4)), 'iscrowd': np.zeros(G, np.int32),
           'num_keypoints': np.zeros(G, np.int32)}
    for g, a in enumerate(annotations):
        out['keypoints'][g] = np.asarray(a['keypoints'], dtype=np.float64).reshape(17, 3)
        out['area'][g] = a['area']
        out['bbox'][g] = a['bbox']
        out['iscrowd'][g] = int(a.get('iscrowd', 0))
        out['num_keypoints'][g] = int(a['num_keypoints'])
    out['ignore'] = (out['iscrowd'] == 1) | (out['num_keypoints'] == 0)
    return out


def detection_order(dets):
    """indices of the detections that are evaluated: argsort(-score, kind='mergesort') cut to MAX_DETS"""
    return np.argsort(-dets['score'], kind='mergesort')[:MAX_DETS]


def oks_matrix(dets, gts):
    """computeOks: the (D, G) float64 object-key-point similarities of the ranked detections (detection_order) and the ground truths; an
    empty array if either side is empty.  The terms exp(-e_i) are added one after the other in ascending key-point order (the
    accumulator below), which is part of the contract: the device entry adds them the same way."""
    gts = ground_truths(gts)
    order = detection_order(dets)
    D, G = len(order), len(gts['area'])
    if D == 0 or G == 0:
        return np.zeros((0, 0))
    kd = dets['keypoints'][order]
    xd, yd = kd[:, :, 0], kd[:, :, 1]
    out = np.zeros((D, G))
    for g in range(G):
        xg, yg, vg = gts['keypoints'][g, :, 0], gts['keypoints'][g, :, 1], gts['keypoints'][g, :, 2]
        k1 = np.count_nonzero(vg > 0)
        if k1 > 0:
            dx = xd - xg
            dy = yd - yg
        else:
            bb = gts['bbox'][g]
            x0, x1, y0, y1 = bb[0] - bb[2], bb[0] + bb[2] * 2, bb[1] - bb[3], bb[1] + bb[3] * 2
            dx = np.maximum(0, x0 - xd) + np.maximum(0, xd - x1)
            dy = np.maximum(0, y0 - yd) + np.maximum(0, yd - y1)
        e = (dx * dx + dy * dy) / KP_VARS / (gts['area'][g] + KP_EPS) / 2
        term = np.exp(-e)
        acc, cnt = np.zeros(D), 0
        for i in range(17):
            if k1 > 0 and not vg[i] > 0:
                continue
            acc = acc + term[:, i]
            cnt += 1
        out[:, g] = acc / cnt
    return out


def evaluate_image(dets, gts, oks=None):
    """evaluateImg for the three area ranges at once.  None if the image has neither detections nor ground truths, else
    {'order' (D,) indices into the input people, 'scores' (D,), 'areas' (D,), 'dt_match' (3, 10, D) int32 file-order index of the matched
    ground truth or -1, 'dt_ig' (3, 10, D) bool, 'gt_ig' (3, G) bool}, D = min(n, MAX_DETS).  `oks`: a matrix to use instead of
    oks_matrix(dets, gts)."""
    gts = ground_truths(gts)
    order = detection_order(dets)
    D, G = len(order), len(gts['area'])
    if D == 0 and G == 0:
        return None
    if oks is None:
        oks = oks_matrix(dets, gts)
    d_area = dets['area'][order]
    crowd = gts['iscrowd'] == 1
    dt_match = np.full((3, len(IOU_THRS), D), -1, dtype=np.int32)
    dt_ig = np.zeros((3, len(IOU_THRS), D), dtype=bool)
    gt_ig = np.zeros((3, G), dtype=bool)
    for a, (lo, hi) in enumerate(AREA_RNGS):
        ig = gts['ignore'] | (gts['area'] < lo) | (gts['area'] > hi)
        gt_ig[a] = ig
        walk = np.argsort(ig, kind='mergesort')
        if D and G:
            for t, thr in enumerate(IOU_THRS):
                matched = np.zeros(G, dtype=bool)
                for d in range(D):
                    iou, m = min(thr, 1 - 1e-10), -1
                    for g in walk:
                        if matched[g] and not crowd[g]:
                            continue
                        if m > -1 and not ig[m] and ig[g]:
                            break
                        if oks[d, g] < iou:
                            continue
                        iou, m = oks[d, g], int(g)
                    if m == -1:
                        continue
                    dt_match[a, t, d] = m
                    dt_ig[a, t, d] = ig[m]
                    matched[m] = True
        outside = (d_area < lo) | (d_area > hi)
        dt_ig[a] |= (dt_match[a] == -1) & outside[None, :]
    return {'order': order.astype(np.int64), 'scores': dets['score'][order], 'areas': d_area, 'dt_match': dt_match, 'dt_ig': dt_ig, 'gt_ig': gt_ig}


def accumulate(per_image):
    """COCOeval.accumulate over the evaluate_image results of a data set (None entries are skipped): (precision (10, 101, 3), recall
    (10, 3)), -1 where an area range has no kept ground truth."""
    per_image = [e for e in per_image if e is not None]
    T, R = len(IOU_THRS), len(REC_THRS)
    precision, recall = -np.ones((T, R, 3)), -np.ones((T, 3))
    for a in range(3):
        if not per_image:
            continue
        scores = np.concatenate([e['scores'] for e in per_image])
        inds = np.argsort(-scores, kind='mergesort')
        match = np.concatenate([e['dt_match'][a] >= 0 for e in per_image], axis=1)[:, inds]
        ig = np.concatenate([e['dt_ig'][a] for e in per_image], axis=1)[:, inds]
        npig = np.count_nonzero(np.concatenate([e['gt_ig'][a] for e in per_image]) == 0)
        if npig == 0:
            continue
        tp_sum = np.cumsum(match & ~ig, axis=1).astype(dtype=float)
        fp_sum = np.cumsum(~match & ~ig, axis=1).astype(dtype=float)
        for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
            nd = len(tp)
            rc = tp / npig
            pr = tp / (fp + tp + KP_EPS)
            q = np.zeros(R)
            recall[t, a] = rc[-1] if nd else 0
            for i in range(nd - 1, 0, -1):
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            idx = np.searchsorted(rc, REC_THRS, side='left')
            for r, pi in enumerate(idx):
                if pi >= nd:
                    break
                q[r] = pr[pi]
            precision[t, :, a] = q
    return precision, recall


def summarize(precision, recall):
    """The ten numbers of COCOeval.summarize for key points, in its order (a dictionary keeps insertion order): each the mean of the
    entries > -1 of its slice, -1 if there is none.  AP50 / AP75 are the thresholds IOU_THRS[0] / IOU_THRS[5]."""
    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0
    out = {}
    for name, s in (('AP', precision), ('AR', recall)):
        out[name] = mean(s[..., 0])
        out[name + '50'] = mean(s[0, ..., 0])
        out[name + '75'] = mean(s[5, ..., 0])
        out[name + '_medium'] = mean(s[..., 1])
        out[name + '_large'] = mean(s[..., 2])
    return out


def results(img_ids, poses_per_image, scores_per_image):
    """The detections in the COCO results format: a list of {'image_id', 'category_id': 1, 'keypoints': [51 numbers], 'score'}, the
    people of every image in the detector's order.  Written to a JSON file, the official tool can score the same detections elsewhere."""
    out = []
    for img_id, poses, scores in zip(img_ids, poses_per_image, scores_per_image):
        d = detections(poses, scores)
        for kp, s in zip(d['keypoints'], d['score']):
            out.append({'image_id': img_id, 'category_id': 1, 'keypoints': [float(v) for v in kp.reshape(-1)], 'score': float(s)})
    return out


def eval_consts():
    """the constant tables as one pmx_eval_consts record (include/pose_mi355x.h): vars[17], iou_thrs[10], area_rngs[3][2], eps, joint[17]"""
    k = np.zeros(1, dtype=EVAL_CONSTS_DTYPE)
    k['vars'], k['iou_thrs'], k['area_rngs'], k['eps'] = KP_VARS, IOU_THRS, np.array(AREA_RNGS, dtype=np.float64), KP_EPS
    k['joint'] = [int(j) for j in params['coco_joint_indices']]
    return k


EVAL_CONSTS_DTYPE = np.dtype([('vars', np.float64, (17,)), ('iou_thrs', np.float64, (10,)), ('area_rngs', np.float64, (3, 2)),
                              ('eps', np.float64), ('joint', np.int32, (17,)), ('reserved', np.int32)])
EVAL_GT_DTYPE = np.dtype([('keypoints', np.float64, (17, 3)), ('area', np.float64), ('bbox', np.float64, (4,)), ('iscrowd', np.int32),
                          ('num_keypoints', np.int32)])      # pmx_eval_gt


def evaluate(ds, det, image_dir, batch=8, img_ids=None, precise=False, on_batch=None):
    """From a detector to its COCO key-point AP: walks the images of the annotation file `ds` (a CocoKeypoints; default every entry of
    ds.images in id order, the images without annotations included -- their detections are false positives, as in the library), `batch`
    at a time through det.evaluate_batch (detection and the per-image evaluation on the device), then accumulate and summarize on the
    host.  -> the ten numbers of summarize plus 'precision', 'recall', 'results' (the COCO results list) and 'per_image'.  An image with
    more than EVAL_MAX_GT annotations is scored by evaluate_image on the host.  on_batch(done, total), if given, is called after every
    batch."""
    from .pose_detector import imread_bgr
    ids = sorted(ds.images) if img_ids is None else list(img_ids)
    batch = int(batch)
    if batch < 1:
        raise ValueError('evaluate: batch = %d' % batch)
    per_image, all_poses, all_scores = [], [], []
    for i in range(0, len(ids), batch):
        chunk = ids[i:i + batch]
        imgs = [imread_bgr(os.path.join(image_dir, ds.file_name(k))) for k in chunk]
        ev, poses, scores = det.evaluate_batch(imgs, [ds.annotations(k) for k in chunk], precise=precise)
        per_image += ev
        all_poses += poses
        all_scores += scores
        if on_batch is not None:
            on_batch(min(i + batch, len(ids)), len(ids))
    precision, recall = accumulate(per_image)
    out = summarize(precision, recall)
    out.update(precision=precision, recall=recall, results=results(ids, all_poses, all_scores), per_image=per_image)
    return out
