"""`FaceDetector` / `HandDetector` -- mirrors of the reference classes (face_detector.py:12-77, hand_detector.py:12-87) on
the same MI355X conv kernels as the pose network (single-branch CPM, models/FaceNet.py / models/HandNet.py).

    FaceDetector(arch='facenet', weights_file=None, model=None, device=-1)(face_img, fast_mode=False) -> 70 key points
    HandDetector(arch='handnet', weights_file=None, model=None, device=-1)(hand_img, fast_mode=False, hand_type="right") -> 21
    FaceDetector.detect_boxes(img, bboxes) / HandDetector.detect_boxes(img, bboxes, hand_types) -> one such list per box of ONE image
    FaceDetector.detect_boxes_batch(imgs, bboxes_per_image) / HandDetector.detect_boxes_batch(imgs, bboxes_per_image, hand_types_per_image)
        -> per image what detect_boxes returns, all boxes of all images in one call (full network batches across image borders)
    detect_person_parts(pose_detector, face_detector, hand_detector, img, poses) -> the face / hand key points of every person (demo.py)
    detect_people_parts(pose_detector, face_detector, hand_detector, imgs, poses_per_image) -> the same for a list of images at once

A key point is `[x, y, confidence]` (ints, np.float32) or `None` when the smoothed maximum does not exceed the threshold,
in the pixel frame of the crop that was passed in -- exactly the reference's return value.  The whole path runs on the
GPU: cv2.resize to 368 x 368 (restated INTER_LINEAR kernel), x / 256 - 0.5, network, corner-aligned resize of the last
stage to the crop size, SciPy-equivalent Gaussian, arg-max (CPU-branch semantics, including the reference's quirk for
tied maxima).  `model=` may be a weights dict or a callable returning the list of stage outputs (test seam; the reference
ignores its `model` argument).
"""
import numpy as np

from . import native
from . import weights as weights_mod
from .entity import params


class _KeypointDetector(object):
    ARCH = None
    SIZE_KEY = None
    THRESH_KEY = None

    def __init__(self, arch=None, weights_file=None, model=None, device=-1, weights=None, max_batch=16, precision='f32'):
        self.arch = arch or self.ARCH
        if self.arch != self.ARCH:
            raise ValueError('%s needs arch=%r' % (type(self).__name__, self.ARCH))
        if int(max_batch) < 1:
            raise ValueError('max_batch must be >= 1')
        if precision not in native.PRECISIONS:
            raise ValueError('precision must be one of %s, got %r' % (', '.join(repr(p) for p in native.PRECISIONS), precision))
        self._precision = precision
        self.device = device
        self.model = model if callable(model) else None
        w = model if isinstance(model, dict) else weights
        if w is None and weights_file:
            w = weights_mod.load_npz(weights_file, self.ARCH)          # serializers.load_npz (face_detector.py:16)
        self._weights = w
        self.max_batch = int(max_batch)       # what detect_boxes may grow the engine to; __call__ alone keeps the batch-1 engine
        self.engine = None
        self._cap = 0
        self._make_engine(1)

    def _make_engine(self, batch):
        # as PoseDetector._make_engine: the state (weights, options, stream, capacities) is taken from the old context, which is destroyed
        # BEFORE the larger one is created; a failed growth rebuilds the previous context and re-raises
        st = None
        if self.engine is not None:
            st = self.engine.state()
            self.engine.close()
            self.engine = None
        try:
            self.engine = self._new_engine(batch, st)
        except Exception:
            self.engine = None
            if st is not None:
                self.engine = self._new_engine(self._cap, st)
            raise
        self._cap = batch

    def _new_engine(self, batch, st):
        size = params[self.SIZE_KEY]
        eng = native.Engine(self.device if self.device >= 0 else 0, max_batch=batch, max_h=size, max_w=size,
                            gaussian_sigma=params['gaussian_sigma'], arch=self.ARCH)
        try:
            if st is not None:
                eng.load_state(st)
            elif self._weights is not None:
                eng.set_weights(self._weights)
            if self._precision != 'f32':
                eng.set_option('precision', native.PRECISIONS[self._precision])
        except Exception:
            eng.close()
            raise
        return eng

    def _grow(self, n):
        """More boxes than the engine's batch: re-create it for min(n, max_batch) crops (larger calls run in chunks of that)."""
        want = min(n, self.max_batch)
        if want > self._cap:
            self._make_engine(want)

    def _detect(self, img, flip_maps=False):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        h, w, _ = img.shape
        size = params[self.SIZE_KEY]
        if self.model is None:
            if self.engine.weights_missing():
                raise RuntimeError('%s has no weights: pass weights_file=, weights= or model=' % type(self).__name__)
            self.engine.forward_u8_resized(img[None], size, size)          # cv2.resize + /256 - 0.5 + network (:31-36)
        else:
            resized = self.engine.resize_u8(img[None], size, size)[0]
            x = np.array(resized[np.newaxis], dtype=np.float32).transpose(0, 3, 1, 2) / 256 - 0.5     # :32
            hs = self.model(x)
            self.engine.set_heat(np.asarray(getattr(hs[-1], 'data', hs[-1]), dtype=np.float32))
        self.engine.set_option('kp_flip_x', int(flip_maps))               # cv2.flip(heatmaps, 1) for left hands (hand_detector.py:46-47)
        kp = self.engine.keypoints(h, w, params[self.THRESH_KEY])[0]      # F.resize_images + peaks (:37-38)
        return _keypoint_list(kp)

    def _detect_boxes(self, img, bboxes, flips):
        """Key points of many boxes of ONE image, one list per box: what `self._detect(crop_image(img, box)[, ::-1])` returns for it.
        All crops are cut, mirrored and resized on the device and run through the network as one batch (chunks of the engine's batch):
        _detect_boxes_batch for a list of one image."""
        if np.ndim(img) != 3 or np.shape(img)[2] != 3:
            raise ValueError('detect_boxes needs one uint8 H x W x 3 image')
        if len(flips) != len(bboxes):
            raise ValueError('one hand type per box')
        return self._detect_boxes_batch([img], [bboxes], [flips])[0]

    def _detect_boxes_batch(self, imgs, bboxes_per_image, flips_per_image):
        """_detect_boxes for the boxes of MANY images (any sizes) in one call: one list per image of one key-point list per box.  The
        crops of all images run through the network in chunks of the engine's batch, taken in box order across image borders."""
        if len(bboxes_per_image) != len(imgs) or len(flips_per_image) != len(imgs):
            raise ValueError('one list of boxes (and of hand types) per image')
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in imgs]
        for im in imgs:
            if im.ndim != 3 or im.shape[2] != 3:
                raise ValueError('detect_boxes_batch needs uint8 H x W x 3 images')
        boxes = []
        for i, (bbs, flips) in enumerate(zip(bboxes_per_image, flips_per_image)):
            if len(flips) != len(bbs):
                raise ValueError('one hand type per box')
            boxes.extend((int(b[0]), int(b[1]), int(b[2]), int(b[3]), int(f), i) for b, f in zip(bbs, flips))
        for k, b in enumerate(boxes):          # (the library checks too; here before the engine may grow)
            if b[2] <= b[0] or b[3] <= b[1]:
                raise native.PmxError(1, 'box %d (image %d): empty (left %d, top %d, right %d, bottom %d)' % ((k, b[5]) + b[:4]))
        counts = [len(bbs) for bbs in bboxes_per_image]
        if not boxes:
            return [[] for _ in imgs]
        thresh = params[self.THRESH_KEY]
        if self.model is None:
            if self.engine.weights_missing():
                raise RuntimeError('%s has no weights: pass weights_file=, weights= or model=' % type(self).__name__)
            self._grow(len(boxes))
            # (an image without boxes is not handed over: the library neither reads nor uploads it)
            kps = self.engine.keypoints_boxes_images([im if n else None for im, n in zip(imgs, counts)], boxes, thresh)
        else:
            # `model=` seam: crops resized on the device one by one, the callable per crop (as __call__), the key points of all crops in
            # chunks of pmx_keypoints_images
            from .pose_detector import PoseDetector
            size = params[self.SIZE_KEY]
            heats = []
            for b in boxes:
                crop = PoseDetector.crop_image(None, imgs[b[5]], b[:4])
                if b[4]:
                    crop = crop[:, ::-1]
                resized = self.engine.resize_u8(np.ascontiguousarray(crop)[None], size, size)[0]
                x = np.array(resized[np.newaxis], dtype=np.float32).transpose(0, 3, 1, 2) / 256 - 0.5
                hs = self.model(x)
                heats.append(np.asarray(getattr(hs[-1], 'data', hs[-1]), dtype=np.float32)[0])
            kps = []
            for k0 in range(0, len(boxes), self.max_batch):
                chunk = boxes[k0:k0 + self.max_batch]
                self._grow(len(chunk))
                self.engine.set_heat(np.stack(heats[k0:k0 + self.max_batch]))
                kps.extend(self.engine.keypoints_images([(b[3] - b[1], b[2] - b[0], b[4]) for b in chunk], thresh))
        out, k = [], 0
        for n in counts:
            out.append([_keypoint_list(kp) for kp in kps[k:k + n]])
            k += n
        return out


def _keypoint_list(kp):
    out = []
    for x, y, conf, valid in kp:
        out.append([int(x), int(y), np.float32(conf)] if valid else None)
    return out


class FaceDetector(_KeypointDetector):
    ARCH, SIZE_KEY, THRESH_KEY = 'facenet', 'face_inference_img_size', 'face_heatmap_peak_thresh'

    def __call__(self, face_img, fast_mode=False):
        """reference face_detector.py:28-40 (`fast_mode` is unused there as well)"""
        return self._detect(face_img)

    def detect_boxes(self, img, bboxes):
        """`[self(PoseDetector.crop_image(img, bbox)) for bbox in bboxes]` in one batched call (boxes (left, top, right, bottom) in image
        pixels, zero padding outside the image): one list of 70 key points (or None) per box, in the box's own pixel frame."""
        return self._detect_boxes(img, bboxes, [0] * len(bboxes))

    def detect_boxes_batch(self, imgs, bboxes_per_image):
        """`[self.detect_boxes(img, bboxes) for img, bboxes in zip(imgs, bboxes_per_image)]` in ONE call: the crops of all images (of
        any sizes) fill the network's batches together."""
        return self._detect_boxes_batch(imgs, bboxes_per_image, [[0] * len(b) for b in bboxes_per_image])


class HandDetector(_KeypointDetector):
    ARCH, SIZE_KEY, THRESH_KEY = 'handnet', 'hand_inference_img_size', 'hand_heatmap_peak_thresh'

    def __call__(self, hand_img, fast_mode=False, hand_type="right"):
        """reference hand_detector.py:28-50: a left hand is mirrored (cv2.flip(img, 1)) before the network and its resized
        heat maps are mirrored back before the Gaussian and the arg-max -- here on the device (the column tables of the
        resize are reversed: the same samples, so also the same row-major order among exactly equal maxima)."""
        hand_img = np.asarray(hand_img)
        if hand_type == "left":
            return self._detect(hand_img[:, ::-1], flip_maps=True)
        return self._detect(hand_img)

    def detect_boxes(self, img, bboxes, hand_types):
        """`[self(PoseDetector.crop_image(img, bbox), hand_type=t) for bbox, t in zip(bboxes, hand_types)]` in one batched call: a left
        hand's crop is mirrored on the device, its maps mirrored back."""
        if len(hand_types) != len(bboxes):
            raise ValueError('one hand type per box')
        return self._detect_boxes(img, bboxes, [1 if t == "left" else 0 for t in hand_types])

    def detect_boxes_batch(self, imgs, bboxes_per_image, hand_types_per_image):
        """`[self.detect_boxes(img, bboxes, types) for img, bboxes, types in zip(...)]` in ONE call: the crops of all images (of any
        sizes) fill the network's batches together."""
        if len(hand_types_per_image) != len(bboxes_per_image) or any(len(t) != len(b) for t, b in zip(hand_types_per_image, bboxes_per_image)):
            raise ValueError('one hand type per box')
        return self._detect_boxes_batch(imgs, bboxes_per_image, [[1 if t == "left" else 0 for t in ts] for ts in hand_types_per_image])


# ---- visualisation / crop helpers of the reference modules (host; cv2.circle / cv2.line rasters are stand-ins).  The two drawing
# functions are the contract of the device form (demo.render_batch: include/pose_mi355x.h::pmx_render) and its oracle in the tests -----
def _shifted(kp, left_top):
    return (kp[0] + left_top[0], kp[1] + left_top[1])


def draw_face_keypoints(orig_img, face_keypoints, left_top):
    """reference face_detector.py:79-97: the 70 key points as radius-2 discs and the `face_line_indices` polylines
    (thickness 1), colour (255, 255, 0), on a copy of the image; `left_top` = origin of the face crop."""
    from .pose_detector import _draw_disc, _draw_line
    img = np.array(orig_img, copy=True)
    for kp in face_keypoints:
        if kp:
            _draw_disc(img, _shifted(kp, left_top), 2, (255, 255, 0))
    for a, b in params['face_line_indices']:
        if face_keypoints[a] and face_keypoints[b]:
            _draw_line(img, _shifted(face_keypoints[a], left_top), _shifted(face_keypoints[b], left_top), (255, 255, 0), 1)
    return img


FINGER_COLORS = [(0, 0, 255), (0, 255, 255), (0, 255, 0), (255, 0, 0), (255, 0, 255)]


def draw_hand_keypoints(orig_img, hand_keypoints, left_top):
    """reference hand_detector.py:89-115: per finger, radius-3 discs at both ends of every bone whose key point exists and
    a thickness-1 line where both exist."""
    from .pose_detector import _draw_disc, _draw_line
    img = np.array(orig_img, copy=True)
    for color, bones in zip(FINGER_COLORS, params['fingers_indices']):
        for a, b in bones:
            ka, kb = hand_keypoints[a], hand_keypoints[b]
            for k in (ka, kb):
                if k:
                    _draw_disc(img, _shifted(k, left_top), 3, color)
            if ka and kb:
                _draw_line(img, _shifted(ka, left_top), _shifted(kb, left_top), color, 1)
    return img


def crop_face(img, rect):
    """reference face_detector.py:99-114 (camera_face_demo.py): `rect` = (x, y, w, h) of a face box; the box is scaled by
    `face_crop_scale` about its centre, clipped to the image and zero-padded to a square.  -> (crop, (left, top))."""
    h, w = img.shape[:2]
    cx, cy = rect[0] + rect[2] / 2, rect[1] + rect[3] / 2
    half_w, half_h = rect[2] * params['face_crop_scale'] / 2, rect[3] * params['face_crop_scale'] / 2
    left, top = max(0, int(cx - half_w)), max(0, int(cy - half_h))
    right, bottom = min(w - 1, int(cx + half_w)), min(h - 1, int(cy + half_h))
    face = img[top:bottom, left:right]
    edge = max(face.shape[:2])
    out = np.zeros((edge, edge, face.shape[2]), dtype=np.uint8)
    out[:face.shape[0], :face.shape[1]] = face
    return out, (left, top)


# ---- demo.py:30-55 for all people of an image at once ---------------------------------------------------------------------------------
def _serial_box_check(bbox):
    """The exception the serial chain raises for a box with no pixels: crop_image's np.zeros for a negative extent, the library for an
    empty crop."""
    if bbox[2] - bbox[0] < 0 or bbox[3] - bbox[1] < 0:
        raise ValueError('negative dimensions are not allowed')
    if bbox[2] == bbox[0] or bbox[3] == bbox[1]:
        raise native.PmxError(1, 'empty crop %r' % (tuple(bbox),))


def _person_boxes(pose_detector, poses):
    """The host half of demo.py:30-55 for the people of one image: (persons, face boxes, their owners, hand boxes, hand types, their
    owners), on a copy of `poses`; raises what the reference's loop would, in (person, face, left, right) order."""
    persons, face_boxes, face_owner, hand_boxes, hand_types, hand_owner = [], [], [], [], [], []
    for p, pose in enumerate(np.array(poses, copy=True)):
        unit = pose_detector.get_unit_length(pose)                       # demo.py:32
        persons.append({'unit_length': unit, 'face': None, 'left': None, 'right': None})
        fb = pose_detector.face_bbox(pose, unit)                          # :36
        if fb is not None:
            _serial_box_check(fb)
            face_boxes.append(fb)
            face_owner.append(p)
        hb = pose_detector.hand_bboxes(pose, unit)                        # :44
        for side in ('left', 'right'):
            if hb[side] is not None:
                _serial_box_check(hb[side])
                hand_boxes.append(hb[side])
                hand_types.append(side)
                hand_owner.append((p, side))
    return persons, face_boxes, face_owner, hand_boxes, hand_types, hand_owner


def _assign_parts(persons, face_owner, face_boxes, face_kps, hand_owner, hand_boxes, hand_kps):
    for p, bbox, kps in zip(face_owner, face_boxes, face_kps):
        persons[p]['face'] = {'bbox': bbox, 'keypoints': kps}
    for (p, side), bbox, kps in zip(hand_owner, hand_boxes, hand_kps):
        persons[p][side] = {'bbox': bbox, 'keypoints': kps}
    return persons


def detect_person_parts(pose_detector, face_detector, hand_detector, img, poses):
    """What the reference demo's loop (demo.py:30-55) computes for every person, with ONE detect_boxes call per detector (two network
    calls however many people).  Per person: {'unit_length', 'face': {'bbox', 'keypoints'} | None, 'left': ..., 'right': ...}.
    Works on a copy of `poses` (the reference's crop_hands moves the wrists in place); every box is computed, and every error the loop
    would raise (e.g. int(nan) for a person without a measurable limb) is raised, before anything runs on the device."""
    persons, face_boxes, face_owner, hand_boxes, hand_types, hand_owner = _person_boxes(pose_detector, poses)
    return _assign_parts(persons, face_owner, face_boxes, face_detector.detect_boxes(img, face_boxes),
                         hand_owner, hand_boxes, hand_detector.detect_boxes(img, hand_boxes, hand_types))


def detect_people_parts(pose_detector, face_detector, hand_detector, imgs, poses_per_image):
    """`[detect_person_parts(pose_detector, face_detector, hand_detector, img, poses) for img, poses in zip(imgs, poses_per_image)]` with
    ONE detect_boxes_batch call per detector for the whole list (images of any sizes): the face crops of all frames fill the face net's
    batches together, the hand crops the hand net's.  Works on copies of the poses; every box of every image is computed, and the first
    error the loop of per-image calls would raise -- in (image, person, face, left, right) order -- is raised, before anything runs on
    the device."""
    if len(poses_per_image) != len(imgs):
        raise ValueError('one array of poses per image')
    per = [_person_boxes(pose_detector, poses) for poses in poses_per_image]
    face_kps = face_detector.detect_boxes_batch(imgs, [b[1] for b in per])
    hand_kps = hand_detector.detect_boxes_batch(imgs, [b[3] for b in per], [b[4] for b in per])
    return [_assign_parts(persons, fo, fb, fk, ho, hb, hk) for (persons, fb, fo, hb, _, ho), fk, hk in zip(per, face_kps, hand_kps)]
