"""CPU: the validation loss (include/pose_mi355x.h: pmx_loss_* / pmx_validate_batch / pmx_get_labels) -- tests/loss_ref.py reproduces what the
reference's own generate_heatmaps / generate_pafs / compute_loss gave (tests/golden/loss_ref.npz, recorded by tools/record_loss_goldens.py),
the eight entries are declared and bound, and the detector's two methods check their arguments before they need a device."""
import os

import numpy as np
import pytest

import loss_ref
from conftest import GOLDEN, pkg

ENTRIES = ('pmx_loss_set_poses', 'pmx_loss_set_targets', 'pmx_loss_enable', 'pmx_loss_get', 'pmx_loss_current_maps', 'pmx_validate_batch',
           'pmx_get_labels', 'pmx_get_loss_targets')
LOSS_CASES = ('generic3', 'axis2', 'empty')          # the 64 x 96 cases: the size of the net_posenet_stage* goldens
MASKS = ('none', 'left', 'all', 'px00', 'pxlast')


@pytest.fixture(scope='module')
def rec():
    z = np.load(os.path.join(GOLDEN, 'loss_ref.npz'))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def stages():
    z = np.load(os.path.join(GOLDEN, 'ref_checks.npz'))
    return [(z['net_posenet_stage%d_paf' % s], z['net_posenet_stage%d_heat' % s]) for s in range(6)]


def mask_of(name, h, w):
    m = np.zeros((h, w), bool)
    if name == 'none':
        return None
    if name == 'left':
        m[:, :w // 2] = True
    elif name == 'all':
        m[:] = True
    elif name == 'px00':
        m[0, 0] = True
    else:
        m[h - 1, w - 1] = True
    return m


@pytest.mark.parametrize('case', ['generic3', 'axis2', 'empty', 'odd'])
def test_loss_ref_labels_equal_the_recorded_reference_labels(rec, case):
    h, w = [int(v) for v in rec[case + '_hw']]
    sigma, width = rec['sigma_width']
    paf, heat = loss_ref.labels((h, w), rec[case + '_poses'], sigma, width)
    assert paf.dtype == np.float32 and heat.dtype == np.float32
    assert np.array_equal(paf, rec[case + '_paf']) and np.array_equal(heat, rec[case + '_heat'])
    if case == 'empty':
        assert not paf.any() and (heat[18] == 1).all() and not heat[:18].any()


@pytest.mark.parametrize('case', LOSS_CASES)
def test_loss_ref_reproduces_the_recorded_compute_loss(rec, stages, case):
    """bound: the reference's F.mean_squared_error is a float32 dot product of N non-negative terms, worst-case relative error N * 2^-24
    (N = elements of the branch); loss_ref sums in float64"""
    for mname in MASKS:
        paf_t, heat_t, mask_t = loss_ref.targets(rec[case + '_paf'], rec[case + '_heat'], mask_of(mname, 64, 96))
        want = rec['%s_%s_loss' % (case, mname)]
        got_total = 0.0
        for s, (yp, yh) in enumerate(stages):
            lp, lh = loss_ref.stage_loss(yp, yh, paf_t[None], heat_t[None], mask_t[None])
            assert abs(lp - want[1 + s]) <= yp.size * 2.0 ** -24 * want[1 + s], (case, mname, s, lp, want[1 + s])
            assert abs(lh - want[7 + s]) <= yh.size * 2.0 ** -24 * want[7 + s], (case, mname, s, lh, want[7 + s])
            got_total += lp + lh
        # the total adds twelve float32 numbers in float32 on top (:68)
        assert abs(got_total - want[0]) <= (stages[0][0].size + 12) * 2.0 ** -24 * want[0], (case, mname, got_total, want[0])
        if mname == 'all':
            assert not want.any()


def test_loss_entries_declared_and_bound():
    native = pkg('native')
    syms = native.header_symbols()
    for s in ENTRIES:
        assert s in syms, s
    assert ('pmx_loss.hip', ['-ffp-contract=off']) in native.SOURCES
    if native.needs_build():
        native.build()
    lib = native.load()
    for s in ENTRIES:
        assert getattr(lib, s) is not None and s in lib._pmx_sig, s
    for name in ('loss_set_poses', 'loss_set_targets', 'loss_enable', 'loss_get', 'loss_current_maps', 'validate_batch', 'labels',
                 'loss_targets'):
        assert callable(getattr(native.Engine, name))
    assert open(native.HEADER).read().count('#define PMX_ABI_VERSION 2') == 1


def _host_detector():
    return object.__new__(pkg('pose_detector').PoseDetector)          # no device context: the checks run before one is needed


def test_validation_loss_checks_its_arguments_without_a_device():
    det = _host_detector()
    img = np.zeros((64, 96, 3), np.uint8)
    one = np.zeros((1, 18, 3))
    bad = [
        ([], [], None),                                               # no image
        ([img.astype(np.float32)], [one], None),                      # not uint8
        ([img, np.zeros((64, 88, 3), np.uint8)], [one, one], None),   # two sizes
        ([np.zeros((60, 96, 3), np.uint8)], [one], None),             # no multiple of 8
        ([img], [one, one], None),                                    # poses for another number of images
        ([img], [np.zeros((1, 17, 3))], None),                        # not 18 joints
        ([img], [one], [np.zeros((8, 12), bool)]),                    # mask of another size
        ([img], [one], [np.zeros((64, 96)), np.zeros((64, 96))]),     # masks for another number of images
    ]
    for imgs, poses, masks in bad:
        with pytest.raises(ValueError):
            det.validation_loss(imgs, poses, masks)
    nan = one.copy()
    nan[0, 3] = (np.nan, 4.0, 2.0)
    with pytest.raises(ValueError):
        det.validation_loss([img], [nan], None)
    nan[0, 3, 2] = 0                                                  # invisible: its position is never read
    imgs, poses, masks = det._check_validation_args([img], [nan], [np.zeros((64, 96), np.uint8)])
    assert poses[0].shape == (1, 18, 3) and masks[0].shape == (64, 96)
    assert det._check_validation_args([img], [[]], None)[1][0].shape == (0, 18, 3)


def test_generate_labels_checks_its_arguments_without_a_device():
    det = _host_detector()
    for shape, poses in (((60, 96), np.zeros((1, 18, 3))), ((64,), np.zeros((1, 18, 3))), ((64, 96), np.zeros((2, 18, 2))),
                         ((0, 96), np.zeros((0, 18, 3))), ((64, 96), 'poses')):
        with pytest.raises(ValueError):
            det.generate_labels(shape, poses)
    inf = np.zeros((1, 18, 3))
    inf[0, 0] = (1.0, np.inf, 1.0)
    with pytest.raises(ValueError):
        det.generate_labels((64, 96), inf)
