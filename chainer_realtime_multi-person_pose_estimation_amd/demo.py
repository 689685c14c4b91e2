"""`python -m <package>.demo --img X [--gpu N] [--out result.png] [--pose-weights P --face-weights F --hand-weights H]` -- the reference's
demo.py (pose, then for every person the face and both hands) on the batched face / hand path: one pose call, then one FaceNet and one
HandNet call for all people of the image (face_hand_detector.detect_person_parts) instead of up to three calls per person.

The canvas is the reference's: cv2.addWeighted(img, 0.6, draw_person_pose(img, poses), 0.4, 0) restated in NumPy (float32 weighted sum,
OpenCV's round-half-even and saturation), then per person the face key points and their white box, the left hand, the right hand, in the
order of the reference's loop (demo.py:30-55).  The weights files are Chainer NPZ files (the reference's models/*.npz).
`--render device` draws the same bytes on the GPU in one launch (render_batch: include/pose_mi355x.h::pmx_render); `render` and its
helpers below stay the default and are that path's contract.
"""
import argparse

import numpy as np

from . import face_hand_detector as fh
from . import pose_detector as pd


def add_weighted(src1, alpha, src2, beta, gamma=0.0):
    """cv2.addWeighted for uint8 images: saturate_cast<uchar>(src1 * alpha + src2 * beta + gamma) in float32, rounded half to even."""
    v = (np.asarray(src1, np.float32) * np.float32(alpha) + np.asarray(src2, np.float32) * np.float32(beta)) + np.float32(gamma)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def draw_rectangle(img, p1, p2, color, thickness=1):
    """cv2.rectangle(img, p1, p2, color, 1) in place: the one-pixel outline of the box with corners p1 and p2 (inclusive), clipped."""
    h, w = img.shape[:2]
    x0, x1 = sorted((int(p1[0]), int(p2[0])))
    y0, y1 = sorted((int(p1[1]), int(p2[1])))
    cx0, cx1, cy0, cy1 = max(x0, 0), min(x1, w - 1), max(y0, 0), min(y1, h - 1)
    if cx0 > cx1 or cy0 > cy1:
        return img
    for y in (y0, y1):
        if 0 <= y < h:
            img[y, cx0:cx1 + 1] = color
    for x in (x0, x1):
        if 0 <= x < w:
            img[cy0:cy1 + 1, x] = color
    return img


def render(img, poses, parts):
    """The reference demo's result image from the poses and detect_person_parts' output."""
    res = add_weighted(img, 0.6, pd.draw_person_pose(img, poses), 0.4, 0)
    for person in parts:
        face = person['face']
        if face is not None:
            b = face['bbox']
            res = fh.draw_face_keypoints(res, face['keypoints'], (b[0], b[1]))
            draw_rectangle(res, (b[0], b[1]), (b[2], b[3]), (255, 255, 255), 1)
        for side in ('left', 'right'):
            hand = person[side]
            if hand is not None:
                b = hand['bbox']
                res = fh.draw_hand_keypoints(res, hand['keypoints'], (b[0], b[1]))
                draw_rectangle(res, (b[0], b[1]), (b[2], b[3]), (255, 255, 255), 1)
    return res


def render_batch(detector, imgs, poses_per_image, parts_per_image):
    """`[render(img, poses, parts) for ...]` for the lists face_hand_detector.detect_people_parts takes and returns, drawn on the device
    in one launch through `detector`'s context (any of the three detectors: drawing needs no weights), byte for byte."""
    if len(parts_per_image) != len(imgs):
        raise ValueError('one list of person parts per image')
    flat = []
    for persons in parts_per_image:
        flat.append([(kind, person[key]['bbox'], person[key]['keypoints'])
                     for person in persons for key, kind in (('face', 'face'), ('left', 'hand'), ('right', 'hand')) if person[key] is not None])
    return detector.engine.render(imgs, poses_per_image, flat, blend=True)


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Pose, face and hand key points of every person in an image')
    parser.add_argument('--img', required=True, help='image file path')
    parser.add_argument('--gpu', '-g', type=int, default=-1, help='GPU ID (negative value selects GPU 0: there is no CPU path)')
    parser.add_argument('--out', '-o', default='result.png', help='output image path')
    parser.add_argument('--pose-weights', default='models/coco_posenet.npz', help='posenet weights (Chainer NPZ)')
    parser.add_argument('--face-weights', default='models/facenet.npz', help='facenet weights (Chainer NPZ)')
    parser.add_argument('--hand-weights', default='models/handnet.npz', help='handnet weights (Chainer NPZ)')
    parser.add_argument('--render', choices=['host', 'device'], default='host',
                        help='where the result image is drawn: host (default, NumPy) or device (one launch; the same bytes)')
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    pose_detector = pd.PoseDetector('posenet', args.pose_weights, device=args.gpu)
    hand_detector = fh.HandDetector('handnet', args.hand_weights, device=args.gpu)
    face_detector = fh.FaceDetector('facenet', args.face_weights, device=args.gpu)
    img = pd.imread_bgr(args.img)
    print('Estimating pose...')
    poses, _ = pose_detector(img)
    print('Estimating face and hand keypoints of %d people...' % len(poses))
    parts = fh.detect_person_parts(pose_detector, face_detector, hand_detector, img, poses)
    res = render_batch(pose_detector, [img], [poses], [parts])[0] if args.render == 'device' else render(img, poses, parts)
    print('Saving result into %s...' % args.out)
    pd.imwrite_bgr(args.out, res)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
