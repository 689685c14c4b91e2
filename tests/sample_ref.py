"""TEST INFRASTRUCTURE -- NumPy restatement of the pixel steps of the reference's sample preparation (coco_data_loader.py:72-205, 334-341).
NOT product code; it lives beside loss_ref.py because oracle/ is frozen.

  resize      cv2.resize (linear, uint8)        <- oracle/resize_ref.py::resize_linear_u8 (the documented "third-party resize unpinned")
  warp_affine cv2.warpAffine, cubic and linear  <- OUR contract, modelled on OpenCV's fixed-point scheme (include/pose_mi355x.h,
                                                   pmx_samples_prepare); no equality with any OpenCV build is claimed
  bgr2hsv / hsv2bgr  cv2.cvtColor               <- OUR contract: OpenCV's integer BGR->HSV tables, a float32 six-sector HSV->BGR
  dilate16    cv2.morphologyEx(MORPH_DILATE, ones((16, 16)))   anchor (8, 8): out[y, x] = max in[y-8 .. y+7, x-8 .. x+7]
  prepare     the whole sample of one SampleRecord (samples.py), step by step on whole images: the FULL rotated image is made and then
              cropped, where the device kernel computes only the crop window

The array functions work on whole images with integer index arrays; warp_pixel is the same contract for ONE pixel in plain Python ints
(tests/test_samples_host.py holds the two against each other).  tools/record_sample_goldens.py gives these functions to the verbatim
reference loader as its cv2 calls."""
import math

import numpy as np

from oracle import precise_ref
from oracle.resize_ref import resize_linear_u8

TAB = 32                      # fractions per pixel
ONE = 32768                   # weight scale


def _fix_sum(w):
    """integer weights -> the same with sum ONE: the largest (first in row-major order among equals) takes the difference"""
    w = [int(v) for v in w]
    big = max(w)
    w[w.index(big)] += ONE - sum(w)
    return w


def _weights(coeffs_1d):
    n = len(coeffs_1d[0])
    tab = np.zeros((TAB, TAB, n * n), np.int32)
    for fy in range(TAB):
        for fx in range(TAB):
            w = [int(np.rint(np.float32(coeffs_1d[fy][i] * coeffs_1d[fx][j]) * np.float32(ONE))) for i in range(n) for j in range(n)]
            tab[fy, fx] = _fix_sum(w)
    return tab


_tables = {}


def cubic_table():
    """(32, 32, 16) int32: weights of the 4 x 4 taps (row-major) per (fy, fx) fraction"""
    if 'c' not in _tables:
        _tables['c'] = _weights([precise_ref._coeffs(np.float32(f) / np.float32(TAB)) for f in range(TAB)])
    return _tables['c']


def linear_table():
    """(32, 32, 4) int32: weights of the 2 x 2 taps"""
    if 'l' not in _tables:
        one = np.float32(1)
        _tables['l'] = _weights([(one - np.float32(f) / np.float32(TAB), np.float32(f) / np.float32(TAB)) for f in range(TAB)])
    return _tables['l']


def rotation_matrix(center, degree, scale=1.0):
    """cv2.getRotationMatrix2D: float64 2 x 3"""
    a = degree * math.pi / 180
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    return np.array([[alpha, beta, (1 - alpha) * center[0] - beta * center[1]],
                     [-beta, alpha, beta * center[0] + (1 - alpha) * center[1]]], np.float64)


def invert_affine(R):
    """the inverse warpAffine uses (float64), as six numbers M0 .. M5"""
    m = [float(v) for v in np.asarray(R, np.float64).ravel()]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0], m[1], m[3], m[4] = A11, m[1] * -D, m[3] * -D, A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def _coords(M, w, h):
    x = np.arange(w, dtype=np.float64)
    y = np.arange(h, dtype=np.float64)
    X = (np.rint((M[1] * y + M[2]) * 1024).astype(np.int64)[:, None] + 16 + np.rint(M[0] * x * 1024).astype(np.int64)[None, :]) >> 5
    Y = (np.rint((M[4] * y + M[5]) * 1024).astype(np.int64)[:, None] + 16 + np.rint(M[3] * x * 1024).astype(np.int64)[None, :]) >> 5
    return X, Y


def warp_affine(img, R, dsize, cubic, border):
    """img (h, w) or (h, w, c) uint8, forward matrix R, dsize (w, h) -> uint8 of that size"""
    img = np.asarray(img, np.uint8)
    flat = img.ndim == 2
    src = (img[:, :, None] if flat else img).astype(np.int64)
    sh, sw = src.shape[:2]
    w, h = int(dsize[0]), int(dsize[1])
    X, Y = _coords(invert_affine(R), w, h)
    sx, fx, sy, fy = X >> 5, X & 31, Y >> 5, Y & 31
    n, k0, tab = (4, -1, cubic_table()) if cubic else (2, 0, linear_table())
    wgt = tab[fy, fx].astype(np.int64)                       # (h, w, n * n)
    acc = np.zeros((h, w, src.shape[2]), np.int64)
    for i in range(n):
        for j in range(n):
            yy, xx = sy + k0 + i, sx + k0 + j
            inside = (yy >= 0) & (yy < sh) & (xx >= 0) & (xx < sw)
            p = np.where(inside[:, :, None], src[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)], int(border))
            acc += wgt[:, :, i * n + j][:, :, None] * p
    out = np.clip((acc + 16384) >> 15, 0, 255).astype(np.uint8)
    return out[:, :, 0] if flat else out


def warp_pixel(img, M, x, y, cubic, border):
    """ONE destination pixel (x, y) of warp_affine from the inverse matrix M, in Python ints: a list of channel values"""
    sh, sw = img.shape[:2]
    X = (int(np.rint((M[1] * float(y) + M[2]) * 1024)) + 16 + int(np.rint(M[0] * float(x) * 1024))) >> 5
    Y = (int(np.rint((M[4] * float(y) + M[5]) * 1024)) + 16 + int(np.rint(M[3] * float(x) * 1024))) >> 5
    n, k0, tab = (4, -1, cubic_table()) if cubic else (2, 0, linear_table())
    w = [int(v) for v in tab[Y & 31, X & 31]]
    chans = 1 if img.ndim == 2 else img.shape[2]
    out = []
    for c in range(chans):
        s = 0
        for i in range(n):
            for j in range(n):
                yy, xx = (Y >> 5) + k0 + i, (X >> 5) + k0 + j
                if 0 <= yy < sh and 0 <= xx < sw:
                    p = int(img[yy, xx] if img.ndim == 2 else img[yy, xx, c])
                else:
                    p = int(border)
                s += w[i * n + j] * p
        out.append(min(max((s + 16384) >> 15, 0), 255))
    return out


# ---- colour ---------------------------------------------------------------------------------------------------------------------
def _div_tables():
    sdiv = np.zeros(256, np.int64)
    hdiv = np.zeros(256, np.int64)
    for i in range(1, 256):
        sdiv[i] = int(np.rint(255 * 4096 / float(i)))
        hdiv[i] = int(np.rint(180 * 4096 / (6.0 * i)))
    return sdiv, hdiv


def bgr2hsv(img):
    """(..., 3) uint8 BGR -> (..., 3) uint8 HSV (H 0 .. 179)"""
    sdiv, hdiv = _div_tables()
    a = np.asarray(img, np.uint8).astype(np.int64)
    b, g, r = a[..., 0], a[..., 1], a[..., 2]
    v = np.maximum(np.maximum(b, g), r)
    d = v - np.minimum(np.minimum(b, g), r)
    s = (d * sdiv[v] + 2048) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (h * hdiv[d] + 2048) >> 12
    h = np.where(h < 0, h + 180, h)
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


def hsv2bgr(hsv):
    """(..., 3) uint8 HSV -> (..., 3) uint8 BGR; a hue >= 180 counts modulo 180"""
    a = np.asarray(hsv, np.uint8).astype(np.int64)
    f32 = np.float32
    h = (a[..., 0] % 180).astype(f32) * f32(6.0 / 180.0)
    s = a[..., 1].astype(f32) * f32(1.0 / 255.0)
    v = a[..., 2].astype(f32) * f32(1.0 / 255.0)
    sec = np.floor(h)
    fr = h - sec
    sec = sec.astype(np.int64)
    bad = (sec < 0) | (sec >= 6)
    sec = np.where(bad, 0, sec)
    fr = np.where(bad, f32(0), fr).astype(f32)
    one = f32(1)
    t = np.stack([v, v * (one - s), v * (one - s * fr), v * (one - s * (one - fr))], axis=-1).astype(f32)
    sector = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    pick = sector[sec]                                                         # (..., 3): which of t for b, g, r
    out = np.take_along_axis(t, pick, axis=-1)
    out = np.where((a[..., 1] == 0)[..., None], v[..., None], out).astype(f32)
    return np.clip(np.rint(out * f32(255)), 0, 255).astype(np.uint8)


def distort(img, deltas):
    """distort_color (:162-173) with the three offsets already drawn (hue -10 .. 10, saturation -40 .. 40, value -30 .. 30)"""
    hsv = bgr2hsv(img).astype(np.int64)
    for c in range(3):
        hsv[..., c] = np.clip(hsv[..., c] + int(deltas[c]), 0, 255)
    return hsv2bgr(hsv.astype(np.uint8))


# ---- mask -----------------------------------------------------------------------------------------------------------------------
def dilate16(mask):
    m = np.asarray(mask) != 0
    h, w = m.shape
    out = np.zeros((h, w), bool)
    for y, x in zip(*np.nonzero(m)):
        out[max(y - 7, 0):min(y + 8, h - 1) + 1, max(x - 7, 0):min(x + 8, w - 1) + 1] = True
    return out


def dilate16_gather(mask):
    """the same from the destination's side: out[y, x] = any in[y-8 .. y+7, x-8 .. x+7]"""
    m = np.asarray(mask) != 0
    h, w = m.shape
    out = np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            out[y, x] = m[max(y - 8, 0):min(y + 7, h - 1) + 1, max(x - 8, 0):min(x + 7, w - 1) + 1].any()
    return out


def resize(img, mask, shape_wh):
    """resize_data's two cv2.resize calls (:76-77): the mask as 0/1 bytes, then != 0"""
    w, h = int(shape_wh[0]), int(shape_wh[1])
    out = resize_linear_u8(img, w, h)
    m = resize_linear_u8(np.asarray(mask != 0, np.uint8)[:, :, None], w, h)[:, :, 0] != 0
    return out, m


def crop(img, mask, offset, insize):
    """random_crop_img's window (:137-157) from its offset: 127 / False outside the image"""
    h, w = img.shape[:2]
    ox, oy = int(offset[0]), int(offset[1])
    out = np.full((insize, insize, 3), 127, np.uint8)
    m = np.zeros((insize, insize), bool)
    for j in range(insize):
        y = j + oy
        if not 0 <= y < h:
            continue
        for i in range(insize):
            x = i + ox
            if 0 <= x < w:
                out[j, i] = img[y, x]
                m[j, i] = mask[y, x]
    return out, m


def prepare(img, mask, rec, insize):
    """one sample of a samples.SampleRecord -> (image (insize, insize, 3) uint8, mask before the dilation, dilated mask)"""
    img = np.ascontiguousarray(img, np.uint8)
    mask = np.zeros(img.shape[:2], bool) if mask is None else np.asarray(mask) != 0
    if rec.resized is not None:
        img, mask = resize(img, mask, rec.resized)
    if rec.R is not None:
        R = np.asarray(rec.R, np.float64)
        size = (int(rec.rotated[0]), int(rec.rotated[1]))
        img = warp_affine(img, R, size, True, 128)
        mask = warp_affine(mask.astype(np.uint8) * 255, R, size, False, 0) > 0
    if rec.offset is not None:
        img, mask = crop(img, mask, rec.offset, insize)
    if rec.distort is not None:
        img = distort(img, rec.distort)
    if rec.flip:
        img, mask = np.ascontiguousarray(img[:, ::-1]), np.ascontiguousarray(mask[:, ::-1])
    img, mask = resize(img, mask, (insize, insize))
    return img, mask, dilate16(mask)
