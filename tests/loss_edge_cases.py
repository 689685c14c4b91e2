"""The case table of the label edge tests (tests/test_loss_edges_host.py on the CPU, tests/test_gpu_loss_edges.py on the device): the poses
crop, rotation and crowds hand to generate_heatmaps / generate_pafs (reference coco_data_loader.py:208-268) all the time and the recorded
pose sets of tests/golden/loss_ref.npz never reach by design -- visible joints outside the image, bands of one limb type that overlap
(count > 1), anti-parallel bands that cancel to exactly 0, v = 1, an invisible person between visible ones, a crowd, paf_width 0, maps
of one row or one column of map pixels.  Pure NumPy, no device code: every input is regenerated from this table, nothing is stored.

A case is CASES[name] = dict(hw=(h, w), poses (n, 18, 3) float64, sigma, width, why).
"""
import numpy as np

from oracle import fixtures as Fx
from oracle.postprocess_ref import LIMBS_POINT

HW = (32, 40)
SIGMA, WIDTH = 3.0, 2.5          # small enough that bands and blobs of a 32 x 40 image stay distinct
REF_SIGMA, REF_WIDTH = 7.0, 8.0  # the reference's own parameters (entity.py:60-61)
NECK, RHIP = 1, 8                # limb 0 runs from the neck to the right hip


def person(nose_xy, hgt, ang=0.0, v=2.0):
    """the template skeleton of oracle/fixtures.py with its nose at nose_xy, body height hgt, turned by ang; every joint visible with v"""
    rot = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
    p = np.empty((18, 3))
    p[:, :2] = Fx._TEMPLATE @ rot.T * hgt + np.asarray(nose_xy, dtype=np.float64)
    p[:, 2] = v
    return p


def turned(p, ang, about):
    """person p turned by ang about the point `about`"""
    rot = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
    q = p.copy()
    q[:, :2] = (p[:, :2] - about) @ rot.T + about
    return q


def bands(shape, poses, width):
    """-> (cover (19, h, w) int: how many people's band of each limb type holds the pixel, margin: the smallest distance of any pixel's
    (hor, ver) to a band edge over all limbs of all people).  Float64, the reference's formulas (generate_constant_paf); the margin is
    `band_margin` of tools/record_loss_goldens.py: only above it can the non-zero pattern of the PAFs be demanded exactly."""
    h, w = shape
    gx, gy = np.meshgrid(np.arange(w), np.arange(h))
    cover, m = np.zeros((len(LIMBS_POINT), h, w), int), np.inf
    for pose in np.asarray(poses, dtype=np.float64).reshape(-1, 18, 3):
        for li, (ja, jb) in enumerate(LIMBS_POINT):
            a, b = pose[ja], pose[jb]
            if not (a[2] > 0 and b[2] > 0) or np.array_equal(a[:2], b[:2]):
                continue
            dist = np.linalg.norm(b[:2] - a[:2])
            unit = (b[:2] - a[:2]) / dist
            hor = unit[0] * (gx - a[0]) + unit[1] * (gy - a[1])
            ver = -unit[1] * (gx - a[0]) + unit[0] * (gy - a[1])
            cover[li] += (0 <= hor) & (hor <= dist) & (np.abs(ver) <= width)
            m = min(m, np.abs(hor).min(), np.abs(hor - dist).min(), np.abs(np.abs(ver) - width).min())
    return cover, m


def axis_person(dx=0, dy=0):
    """integer coordinates, every limb horizontal or vertical, inside 32 x 40 (the idea of axis_people in tools/record_loss_goldens.py)"""
    a = {0: (20, 4), 1: (20, 10), 2: (14, 10), 3: (14, 16), 4: (10, 16), 5: (27, 10), 6: (27, 17), 7: (31, 17), 8: (20, 18), 9: (20, 24),
         10: (15, 24), 11: (20, 15), 12: (26, 15), 13: (26, 22), 14: (14, 4), 15: (27, 4), 16: (14, 3), 17: (27, 3)}
    p = np.zeros((18, 3))
    for j, (x, y) in a.items():
        p[j] = (x + dx, y + dy, 2)
    for ja, jb in LIMBS_POINT:
        assert p[ja, 0] == p[jb, 0] or p[ja, 1] == p[jb, 1]
    return p


def _crowd(n, seed):
    """n small people all over the image and a little beyond it, each joint visible (v = 1 or 2) with probability 0.85"""
    rng = np.random.default_rng(seed)
    h, w = HW
    out = []
    for _ in range(n):
        p = person((rng.uniform(-3, w + 3), rng.uniform(-3, h - 5)), rng.uniform(8, 20), rng.uniform(-0.6, 0.6))
        p[:, 2] = np.where(rng.uniform(size=18) < 0.85, rng.integers(1, 3, 18), 0)
        out.append(p)
    return np.array(out)


def _tiny_limb():
    """right shoulder and right elbow 1e-3 apart, placed so that pixel (12, 9) lies 0.4e-3 along the 1e-3 long band"""
    p = person((18.3, 3.2), 24.7, 0.07)
    u = np.array([np.cos(0.3), np.sin(0.3)])
    p[2, :2] = np.array([12.0, 9.0]) - 0.4e-3 * u + 0.3 * np.array([-u[1], u[0]])
    p[3, :2] = p[2, :2] + 1e-3 * u
    return p[None]


def _cases():
    c = {}

    def add(name, hw, poses, sigma, width, why):
        c[name] = dict(hw=hw, poses=np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 18, 3)), sigma=float(sigma),
                       width=float(width), why=why)

    add('outside4', HW, [person((6.3, -4.2), 24.7, 0.2), person((33.6, 11.4), 26.3, -0.25)], SIGMA, WIDTH,
        'visible joints beyond each of the four image sides, limbs that cross a border')
    add('far', HW, [person((320.4, 6.3), 22.1)], REF_SIGMA, REF_WIDTH, 'a person 300 px to the right: no PAF, heat 0, background 1 in float32')
    a = person((19.3, 3.4), 25.6, 0.1)
    add('parallel2', HW, [a, a], SIGMA, WIDTH, 'two identical people: every band pixel has count 2')
    b = a.copy()
    b[[NECK, RHIP]] = a[[RHIP, NECK]]
    add('anti', HW, [a, b], SIGMA, WIDTH, 'neck and right hip swapped: limb 0 is exactly 0 where both bands hold the pixel')
    a = person((17.2, 4.3), 24.3, 0.05)
    add('cross', HW, [a, turned(a, np.pi / 3, (a[NECK, :2] + a[RHIP, :2]) / 2)], SIGMA, WIDTH, 'the same limb of two people crossing at 60 degrees')
    a, b = person((14.6, 2.7), 23.9, -0.1, v=1.0), person((25.3, 5.8), 21.4, 0.15, v=1.0)
    a[4, :2] = a[3, :2]
    add('coincident_v1', HW, [a, b], SIGMA, WIDTH, 'right hand on right elbow at non-integer coordinates, every v = 1')
    add('invisible_between', HW, [person((11.7, 3.1), 24.2, 0.1), person((19.4, 4.6), 23.3, -0.05, v=0.0), person((27.9, 2.4), 25.1, -0.12)],
        SIGMA, WIDTH, 'three people, the middle one with every v = 0')
    add('crowd24', HW, _crowd(24, 2407), SIGMA, WIDTH, 'the person loop at crowd length')
    add('width0', HW, [axis_person(), axis_person(8, 7)], 2, 0, 'paf_width 0 on integer-axis limbs: only pixels on the segment are set')
    add('row8', (8, 40), [person((4.2, 3.6), 14.0, 0.07 - np.pi / 2), person((36.4, 3.9), 12.5, np.pi / 2 - 0.05)], 2, 1.5,
        'one row of map pixels: the grid builder\'s div == 0 branch in y')
    add('col8', (40, 8), [person((3.7, 2.3), 15.2, 0.04), person((3.9, 37.2), 14.1, np.pi - 0.06)], 2, 1.5, 'one column of map pixels: div == 0 in x')
    add('one8', (8, 8), [person((3.4, 1.2), 6.1, 0.1)], 2, 1.5, 'one map pixel: every corner weight is (1, 0, 0, 0)')
    add('tiny_limb', HW, _tiny_limb(), SIGMA, WIDTH, 'two joints 1e-3 apart')
    return c


CASES = _cases()
NAMES = tuple(CASES)
INTEGER_AXES = ('width0',)             # limbs on integer axes: pixels lie exactly ON band edges, no margin to demand
