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

The mask contract restates `annToMask` of the library's C part (rleFrPoly + rleMerge + rleDecode) from its published source.  The library
is not a dependency and the restatement has not been compared with it bit for bit: that pin is open.
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
