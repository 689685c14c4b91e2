"""Records tests/golden/sample_ref.npz: what the reference's own data loader makes of small seeded inputs, for the sample-preparation tests.

Run once where the reference is present (oracle/_refimport.py::REFERENCE_DIR):  python tools/record_sample_goldens.py

The reference's coco_data_loader.py is imported VERBATIM on top of oracle._refimport's stand-in modules.  Its cv2 calls that the stand-in
module lacks (getRotationMatrix2D, warpAffine, cvtColor, morphologyEx, the constants, and resize of a one-channel array) are added here,
implemented by tests/sample_ref.py: OpenCV is not installable, so the PIXEL arithmetic of the goldens is that restatement's.  What the
goldens pin to the reference's own code is the ORCHESTRATION: the order of the random draws, the int32 truncation of the poses, the crop
arithmetic with its eight bounds, the joint swaps, the 127 / 128 seam, the dilation after the resize.  The draws are captured by wrapping
the `random` / `np.random` calls.  Only inputs and results are stored; nothing of the reference's text.
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import _refimport as R          # noqa: E402
import sample_ref                           # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
INSIZE = 32
N_SEEDS = 24
LABEL_SEEDS = (0, 5)                        # the seeds whose label maps are stored (57 x 32 x 32 float32 each)
MISSING = -999


def _install_cv2():
    cv2 = sys.modules['cv2']
    plain_resize = R._cv2_resize

    def resize(src, dsize, *a, **k):
        src = np.asarray(src)
        if src.ndim == 2:
            return plain_resize(src[:, :, None], dsize, *a, **k)[:, :, 0]
        return plain_resize(src, dsize, *a, **k)

    def warp_affine(src, M, dsize, flags=1, borderMode=0, borderValue=0):
        assert flags in (cv2.INTER_LINEAR, cv2.INTER_CUBIC) and borderMode == cv2.BORDER_CONSTANT
        b = np.atleast_1d(np.asarray(borderValue, np.float64))
        assert (b == b[0]).all()
        return sample_ref.warp_affine(src, M, dsize, flags == cv2.INTER_CUBIC, int(np.rint(b[0])))

    def cvt_color(src, code):
        return sample_ref.bgr2hsv(src) if code == cv2.COLOR_BGR2HSV else sample_ref.hsv2bgr(src)

    def morphology_ex(src, op, kernel):
        assert op == cv2.MORPH_DILATE and kernel.shape == (16, 16) and (kernel == 1).all()
        return sample_ref.dilate16(src).astype(np.uint8)

    cv2.__dict__.update(resize=resize, getRotationMatrix2D=sample_ref.rotation_matrix, warpAffine=warp_affine, cvtColor=cvt_color,
                        morphologyEx=morphology_ex, BORDER_CONSTANT=0, COLOR_BGR2HSV=40, COLOR_HSV2BGR=54, MORPH_DILATE=1)
    return cv2


_loader = None


def reference_loader():
    global _loader
    if _loader is None:
        CDL = R.import_reference_modules()['coco_data_loader']
        _install_cv2()
        _loader = object.__new__(CDL.CocoDataLoader)
        _loader.insize = INSIZE
        _loader.mode = 'train'
    return _loader


class Capture(object):
    """wraps the random calls augment_data makes and the loader's resize_data / generate_heatmaps while one sample is made"""

    def __enter__(self):
        self.log = []
        self.saved = (random.random, random.choice, np.random.randn, np.random.rand, np.random.randint)
        r_random, r_choice, n_randn, n_rand, n_randint = self.saved
        log = self.log

        def choice(seq):
            i = r_choice(range(len(seq)))          # the same draw as random.choice(seq): one _randbelow(len(seq))
            log.append(('choice', i))
            return seq[i]

        def wrap(name, fn):
            def f(*a):
                v = fn(*a)
                log.append((name, v))
                return v
            return f
        random.random, random.choice = wrap('random', r_random), choice
        np.random.randn, np.random.rand, np.random.randint = wrap('randn', n_randn), wrap('rand', n_rand), wrap('randint', n_randint)
        return self

    def __exit__(self, *exc):
        random.random, random.choice, np.random.randn, np.random.rand, np.random.randint = self.saved
        return False


def run_reference(img, mask, poses, seed):
    """generate_labels of the verbatim loader after seeding both generators -> dict of draws and results"""
    gen = reference_loader()
    cv2 = sys.modules['cv2']
    seen = {}
    orig_resize_data, orig_heat, orig_warp = gen.resize_data, gen.generate_heatmaps, cv2.warpAffine

    def resize_data(i, m, p, shape):
        seen.setdefault('shapes', []).append(tuple(int(v) for v in shape))
        return orig_resize_data(i, m, p, shape)

    def heat(i, p, sigma):
        seen['poses'] = np.array(p, dtype=np.int32)
        assert np.asarray(p).dtype == np.int32
        return orig_heat(i, p, sigma)

    def warp(src, M, dsize, **k):
        if 'R' not in seen:
            seen['R'], seen['rotated'] = np.array(M, np.float64), tuple(int(v) for v in dsize)
        return orig_warp(src, M, dsize, **k)

    random.seed(seed)
    np.random.seed(seed)
    gen.__dict__.update(resize_data=resize_data, generate_heatmaps=heat)
    cv2.warpAffine = warp
    try:
        with Capture() as cap:
            out_img, pafs, heats, out_mask = gen.generate_labels(img.copy(), poses.copy(), mask.copy())
    finally:
        del gen.__dict__['resize_data'], gen.__dict__['generate_heatmaps']
        cv2.warpAffine = orig_warp
    log = cap.log
    names = [n for n, _ in log]
    assert names[:4] == ['random', 'randn', 'choice', 'rand'] and names[4] == 'randint', names
    distort = [MISSING] * 3
    k = 5
    if log[4][1]:
        assert names[5:8] == ['randint'] * 3
        distort = [int(log[5 + c][1]) - lo for c, lo in enumerate((10, 40, 30))]
        k = 8
    assert names[k:] == ['randint'], names
    return dict(u=float(log[0][1]), randn=float(log[1][1]), index=int(log[2][1]), r_xy=np.array(log[3][1], np.float64),
                distort=np.array(distort, np.int32), flip=int(log[k][1]), resized=np.array(seen['shapes'][0], np.int32),
                R=seen['R'], rotated=np.array(seen['rotated'], np.int32), poses=seen['poses'], img=out_img, mask=np.asarray(out_mask, bool),
                pafs=pafs, heats=heats)


def run_reference_val(img, mask, poses):
    """validation mode: resize_data to insize x insize and the dilation of generate_labels (:336, :340)"""
    gen = reference_loader()
    cv2 = sys.modules['cv2']
    out_img, m, p = gen.resize_data(img.copy(), mask.copy(), poses.copy(), shape=(INSIZE, INSIZE))
    m = cv2.morphologyEx(m.astype('uint8'), cv2.MORPH_DILATE, np.ones((16, 16))).astype('bool')
    return out_img, m, np.array(p, np.int32)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def make_inputs():
    """four small scenes (image <= 64 pixels a side, mask with set pixels on the border, int32 poses).  Poses are numbers: scene 2 has only a
    person far larger than the image (bounding box > 128: min_scale at its lower clamp) and scene 3 one above 512 (max_scale at 1)."""
    rng = np.random.default_rng(20240)
    scenes = []
    for h, w, spans in ((48, 64, [(8, 4, 40, 36)]), (64, 40, [(4, 6, 30, 50), (10, 20, 38, 60)]), (56, 56, [(-60, -50, 110, 120)]),
                        (40, 60, [(-250, -200, 300, 260), (10, 8, 44, 30)])):
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(xx * 4 + yy) % 256, (yy * 5 + 30) % 256, (xx * 2 + yy * 3) % 256], axis=-1) + rng.integers(-20, 21, (h, w, 3))
        img = np.clip(img, 0, 255).astype(np.uint8)
        mask = np.zeros((h, w), bool)
        mask[0:5, 0:7] = True
        mask[h - 3:, w // 2:w // 2 + 9] = True
        mask[h // 2:h // 2 + 6, w - 2:] = True
        poses = np.zeros((len(spans), 18, 3), np.int32)
        for p, (x1, y1, x2, y2) in enumerate(spans):
            poses[p, :, 0] = rng.integers(x1, x2 + 1, 18)
            poses[p, :, 1] = rng.integers(y1, y2 + 1, 18)
            poses[p, :, 2] = rng.choice([0, 1, 2], 18, p=[0.15, 0.25, 0.6])
            poses[p, 0] = (x1, y1, 2)
            poses[p, 1] = (x2, y2, 2)
        scenes.append((img, mask, poses))
    return scenes


def main():
    assert R.reference_available()
    from conftest import pkg
    S = pkg('samples')
    scenes = make_inputs()
    out = {'insize': np.array(INSIZE, np.int32), 'n_seeds': np.array(N_SEEDS, np.int32), 'n_scenes': np.array(len(scenes), np.int32),
           'label_seeds': np.array(LABEL_SEEDS, np.int32)}
    for i, (img, mask, poses) in enumerate(scenes):
        out['scene%d_img' % i], out['scene%d_mask' % i], out['scene%d_poses' % i] = img, mask, poses
        vi, vm, vp = run_reference_val(img, mask, poses)
        out['val%d_img' % i], out['val%d_mask' % i], out['val%d_poses' % i] = vi, vm, vp
    cover = dict(distort=0, plain=0, flip=0, noflip=0, left=0, top=0, right=0, bottom=0, min_lo=0, min_hi=0, max_lo=0, max_hi=0)
    for seed in range(N_SEEDS):
        img, mask, poses = scenes[seed % len(scenes)]
        ref = run_reference(img, mask, poses, seed)
        random.seed(seed)
        np.random.seed(seed)
        rec = S.draw_augmentation(img.shape[:2], poses, INSIZE)
        d = rec.draws
        assert d['u'] == ref['u'] and d['randn'] == ref['randn'] and d['bbox_index'] == ref['index'] and tuple(ref['r_xy']) == d['r_xy']
        assert tuple(ref['resized']) == rec.resized and tuple(ref['rotated']) == rec.rotated and np.array_equal(ref['R'], rec.R)
        assert (rec.distort is None) == (ref['distort'][0] == MISSING) and (rec.distort is None or tuple(ref['distort']) == rec.distort)
        assert rec.flip == bool(ref['flip'])
        assert np.array_equal(S.transform_poses(poses, rec), ref['poses'])
        got = sample_ref.prepare(img, mask, rec, INSIZE)
        assert np.array_equal(got[0], ref['img']) and np.array_equal(got[2], ref['mask']), seed
        x1, y1, x2, y2, x_from, y_from, x_to, y_to = d['bounds']
        for name, hit in (('distort', rec.distort is not None), ('plain', rec.distort is None), ('flip', rec.flip), ('noflip', not rec.flip),
                          ('left', x_from > 0), ('top', y_from > 0), ('right', x_to < INSIZE - 1), ('bottom', y_to < INSIZE - 1),
                          ('min_lo', d['min_scale'] == 0.5), ('min_hi', d['min_scale'] == 1), ('max_lo', d['max_scale'] == 1),
                          ('max_hi', d['max_scale'] == 2.0)):
            cover[name] += bool(hit)
        pre = 'seed%d_' % seed
        for k in ('u', 'randn', 'index', 'r_xy', 'distort', 'flip', 'resized', 'R', 'rotated', 'poses', 'img', 'mask'):
            out[pre + k] = np.asarray(ref[k])
        out[pre + 'scales'] = np.array([d['min_scale'], d['max_scale'], d['scale']], np.float64)
        out[pre + 'center_offset'] = np.array(list(d['center']) + list(rec.offset), np.int32)
        out[pre + 'bounds'] = np.array(d['bounds'], np.int32)
        if seed in LABEL_SEEDS:
            out[pre + 'pafs'], out[pre + 'heats'] = ref['pafs'], ref['heats']
    print(cover)
    assert min(cover.values()) >= 2, cover
    path = os.path.join(GOLDEN, 'sample_ref.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f != 'sample_ref.npz')
    print(path, size, 'bytes (largest other golden: %d)' % largest)
    assert size <= largest and size <= 1 << 20


if __name__ == '__main__':
    main()
