"""Host side of the sample preparation (reference coco_data_loader.py:61-205, 334-341): the numbers of one sample.

The pixels of a sample are made on the device (csrc/pmx_samples.hip, `PoseDetector.prepare_samples`); what is left for the host is a few
dozen numbers per sample, computed here in float64 / int32 NumPy exactly as the reference computes them:

  SampleRecord        every step of one sample as plain numbers; a step that is None / False does not happen.  mode 'val' = only the
                      final resize to insize x insize (step 6 of generate_labels)
  draw_augmentation   the reference's random policy: consumes `random` and `np.random` in its order and with its calls, so that after
                      random.seed(k); np.random.seed(k) it arrives at the numbers augment_data (:195-205) would use
  transform_poses     the int32 poses after all steps, with the reference's truncations (`poses` is an int32 array,
                      parse_coco_annotation :313, so every float assigned into it is cut toward zero) and joint swaps
"""
import math
import random

import numpy as np

from .entity import JointType

# training keys of the reference's params (entity.py:63-68)
AUG = dict(min_box_size=64, max_box_size=512, min_scale=0.5, max_scale=2.0, max_rotate_degree=40, center_perterb_max=40)
# distort_color's offsets (:167-169): value = -lo + randint(2 * lo + 1)
DISTORT_RANGE = (10, 40, 30)
SWAPS = [(JointType.LeftEye, JointType.RightEye), (JointType.LeftEar, JointType.RightEar), (JointType.LeftShoulder, JointType.RightShoulder),
         (JointType.LeftElbow, JointType.RightElbow), (JointType.LeftHand, JointType.RightHand), (JointType.LeftWaist, JointType.RightWaist),
         (JointType.LeftKnee, JointType.RightKnee), (JointType.LeftFoot, JointType.RightFoot)]


class SampleRecord(object):
    """One sample as plain numbers.  src_hw: the source size; resized: (w, h) of random_resize_img or None; R: forward 2 x 3 matrix of
    random_rotate_img (float64) with `rotated` = (w, h) of the rotated image, or None; offset: (x, y) of the crop window's first pixel in
    the (rotated) image, or None; distort: three HSV offsets or None; flip.  The draw_* fields only document a drawn record."""

    def __init__(self, src_hw, insize, mode='train', resized=None, R=None, rotated=None, offset=None, distort=None, flip=False, **draws):
        if mode not in ('train', 'val'):
            raise ValueError("SampleRecord: mode must be 'train' or 'val'")
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        self.insize = int(insize)
        self.mode = mode
        self.resized = None if resized is None else (int(resized[0]), int(resized[1]))
        self.R = None if R is None else np.array(R, np.float64).reshape(2, 3)
        self.rotated = None if rotated is None else (int(rotated[0]), int(rotated[1]))
        self.offset = None if offset is None else (int(offset[0]), int(offset[1]))
        self.distort = None if distort is None else tuple(int(v) for v in distort)
        self.flip = bool(flip)
        self.draws = draws
        self.check()

    @classmethod
    def val(cls, src_hw, insize):
        return cls(src_hw, insize, mode='val')

    def check(self):
        h, w = self.src_hw
        if h < 1 or w < 1:
            raise ValueError('SampleRecord: source size %r' % (self.src_hw,))
        if self.insize < 8 or self.insize % 8:
            raise ValueError('SampleRecord: insize %d must be a positive multiple of 8' % self.insize)
        if self.resized is not None and min(self.resized) < 1:
            raise ValueError('SampleRecord: resized size %r' % (self.resized,))
        if (self.R is None) != (self.rotated is None):
            raise ValueError('SampleRecord: R and rotated go together')
        if self.R is not None:
            if not np.isfinite(self.R).all() or self.R[0, 0] * self.R[1, 1] - self.R[0, 1] * self.R[1, 0] == 0:
                raise ValueError('SampleRecord: R must be finite and invertible')
            if min(self.rotated) < 1:
                raise ValueError('SampleRecord: rotated size %r' % (self.rotated,))
        if self.distort is not None:
            if len(self.distort) != 3 or any(abs(d) > r for d, r in zip(self.distort, DISTORT_RANGE)):
                raise ValueError('SampleRecord: distort %r outside +-%r' % (self.distort, DISTORT_RANGE))
        if self.mode == 'val':
            if not (self.resized is None and self.R is None and self.offset is None and self.distort is None and not self.flip):
                raise ValueError("SampleRecord: mode 'val' has only the final resize")
        elif self.offset is None:
            raise ValueError("SampleRecord: mode 'train' needs the crop offset (the crop makes the insize x insize window)")

    def size_before_crop(self):
        """(w, h) of the image the crop window is cut from"""
        if self.rotated is not None:
            return self.rotated
        if self.resized is not None:
            return self.resized
        return (self.src_hw[1], self.src_hw[0])


def rotation_matrix(center, degree, scale=1.0):
    """cv2.getRotationMatrix2D(center, degree, scale) in float64"""
    a = degree * math.pi / 180
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    return np.array([[alpha, beta, (1 - alpha) * center[0] - beta * center[1]],
                     [-beta, alpha, beta * center[0] + (1 - alpha) * center[1]]], np.float64)


def invert_affine(R):
    """The six float64 numbers of the inverse of a 2 x 3 affine matrix, computed as cv2.warpAffine inverts its argument."""
    m = [float(v) for v in np.asarray(R, np.float64).reshape(6)]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0], m[1], m[3], m[4] = A11, m[1] * -D, m[3] * -D, A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def check_int_poses(poses, what='poses'):
    p = np.asarray(poses)
    if p.ndim != 3 or p.shape[1:] != (len(JointType), 3):
        raise ValueError('%s: expected (n, 18, 3), got %r' % (what, p.shape))
    if p.dtype.kind not in 'iu':
        if not np.isfinite(p).all() or (p != np.trunc(p)).any():
            raise ValueError('%s: the reference keeps poses as int32 (parse_coco_annotation); got non-integer values' % what)
    return np.array(p, dtype=np.int32)


def pose_bboxes(poses):
    """get_pose_bboxes (:61-70): per person (x1, y1, x2, y2) of the joints with v > 0"""
    out = []
    for pose in poses:
        vis = pose[pose[:, 2] > 0]
        if not len(vis):
            raise ValueError('a person without a visible joint has no bounding box (the reference fails there too)')
        out.append([vis[:, 0].min(), vis[:, 1].min(), vis[:, 0].max(), vis[:, 1].max()])
    return np.array(out)


def _resize_poses(poses, shape_wh, size_wh):
    poses[:, :, :2] = (poses[:, :, :2] * np.array(shape_wh) / np.array(size_wh))          # :78, into int32
    return poses


def _rotate_poses(poses, R):
    tmp = np.ones_like(poses)
    tmp[:, :, :2] = poses[:, :, :2].copy()
    rot = np.dot(tmp, R.T)                                                                # :121
    out = poses.copy()
    out[:, :, :2] = rot                                                                   # :123, into int32
    return out


def _flip_poses(poses, w):
    poses[:, :, 0] = w - 1 - poses[:, :, 0]
    for a, b in SWAPS:
        tmp = poses[:, a].copy()
        poses[:, a] = poses[:, b]
        poses[:, b] = tmp
    return poses


def transform_poses(poses, rec):
    """int32 poses (n, 18, 3) in source pixels -> int32 poses in the pixels of the prepared insize x insize sample"""
    p = check_int_poses(poses).copy()
    h, w = rec.src_hw
    if rec.resized is not None:
        p = _resize_poses(p, rec.resized, (w, h))
        w, h = rec.resized
    if rec.R is not None:
        p = _rotate_poses(p, rec.R)
        w, h = rec.rotated
    if rec.offset is not None:
        p[:, :, :2] -= np.array(rec.offset, dtype=np.int32)
        w, h = rec.insize, rec.insize
    if rec.flip:
        p = _flip_poses(p, w)
    return _resize_poses(p, (rec.insize, rec.insize), (w, h))                             # :336


def draw_augmentation(shape_hw, poses, insize):
    """The record augment_data (:195-205) would use for an image of shape_hw with these int32 poses, drawn from `random` / `np.random`."""
    h, w = int(shape_hw[0]), int(shape_hw[1])
    p = check_int_poses(poses).copy()
    if not len(p):
        raise ValueError('draw_augmentation: no person (random_resize_img needs a bounding box)')
    # random_resize_img (:81-103)
    boxes = pose_bboxes(p)
    sizes = ((boxes[:, 2:] - boxes[:, :2] + 1) ** 2).sum(axis=1) ** 0.5
    min_scale = AUG['min_box_size'] / sizes.min()
    max_scale = AUG['max_box_size'] / sizes.max()
    min_scale = min(max(min_scale, AUG['min_scale']), 1)
    max_scale = min(max(max_scale, 1), AUG['max_scale'])
    u = random.random()
    scale = float((max_scale - min_scale) * u + min_scale)
    resized = (round(w * scale), round(h * scale))
    p = _resize_poses(p, resized, (w, h))
    w, h = resized
    # random_rotate_img (:105-124)
    randn = np.random.randn()
    degree = randn / 3 * AUG['max_rotate_degree']
    rad = degree * math.pi / 180
    center = (w / 2, h / 2)
    R = rotation_matrix(center, degree, 1)
    bbox = (w * abs(math.cos(rad)) + h * abs(math.sin(rad)), w * abs(math.sin(rad)) + h * abs(math.cos(rad)))
    R[0, 2] += bbox[0] / 2 - center[0]
    R[1, 2] += bbox[1] / 2 - center[1]
    rotated = (int(bbox[0] + 0.5), int(bbox[1] + 0.5))
    p = _rotate_poses(p, R)
    w, h = rotated
    # random_crop_img (:126-160)
    boxes = pose_bboxes(p)
    index = random.choice(range(len(boxes)))
    box = boxes[index]
    box_center = box[:2] + (box[2:] - box[:2]) / 2
    r_xy = np.random.rand(2)
    perturb = (r_xy - 0.5) * 2 * AUG['center_perterb_max']
    c = (box_center + perturb + 0.5).astype('i')
    offset = (c - (insize - 1) / 2 + 0.5).astype('i')
    offset_ = (c + (insize - 1) / 2 - (w - 1, h - 1) + 0.5).astype('i')
    x1, y1 = (c - (insize - 1) / 2 + 0.5).astype('i')
    x2, y2 = (c + (insize - 1) / 2 + 0.5).astype('i')
    x1, y1, x2, y2 = max(x1, 0), max(y1, 0), min(x2, w - 1), min(y2, h - 1)
    x_from = -offset[0] if offset[0] < 0 else 0
    y_from = -offset[1] if offset[1] < 0 else 0
    x_to = insize - offset_[0] - 1 if offset_[0] >= 0 else insize - 1
    y_to = insize - offset_[1] - 1 if offset_[1] >= 0 else insize - 1
    bounds = [int(v) for v in (x1, y1, x2, y2, x_from, y_from, x_to, y_to)]
    # distort_color (:162-173), flip_img (:175-193)
    distort = None
    if np.random.randint(2):
        distort = tuple(int(-r + np.random.randint(2 * r + 1)) for r in DISTORT_RANGE)
    flip = bool(np.random.randint(2))
    return SampleRecord((int(shape_hw[0]), int(shape_hw[1])), insize, 'train', resized=resized, R=R, rotated=rotated,
                        offset=(int(offset[0]), int(offset[1])), distort=distort, flip=flip,
                        scale=scale, min_scale=float(min_scale), max_scale=float(max_scale), u=float(u), randn=float(randn), degree=float(degree),
                        bbox_index=int(index), r_xy=(float(r_xy[0]), float(r_xy[1])), center=(int(c[0]), int(c[1])), bounds=bounds)
