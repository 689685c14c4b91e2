"""CPU: the case table tests/loss_edge_cases.py does what each case is built for (asserted on the NumPy restatement tests/loss_ref.py
alone), tests/loss_ref.py::labels equals the verbatim reference's generate_pafs / generate_heatmaps bit for bit on every case (live,
where the reference is present: no golden of full label maps is stored), and tests/loss_ref.py::targets on maps of one row / column /
pixel is what the corner-aligned resize says it is.  The device half is tests/test_gpu_loss_edges.py."""
import numpy as np
import pytest

import loss_edge_cases as E
import loss_ref
from oracle import _refimport as R
from oracle.postprocess_ref import LIMBS_POINT


@pytest.fixture(scope='module')
def lab():
    """loss_ref.labels of every case: computed once, never modified"""
    return {n: loss_ref.labels(c['hw'], c['poses'], c['sigma'], c['width']) for n, c in E.CASES.items()}


def test_the_table_holds_the_cases_the_device_file_needs():
    for n in ('outside4', 'far', 'parallel2', 'anti', 'cross', 'coincident_v1', 'invisible_between', 'crowd24', 'width0', 'row8', 'col8',
              'tiny_limb'):
        assert n in E.CASES
    assert E.CASES['row8']['hw'] == (8, 40) and E.CASES['col8']['hw'] == (40, 8) and E.CASES['one8']['hw'] == (8, 8)
    assert len(E.CASES['crowd24']['poses']) == 24 and len(E.CASES['invisible_between']['poses']) == 3
    assert E.CASES['width0']['width'] == 0 and E.CASES['width0']['sigma'] == 2
    for n in ('row8', 'col8'):
        assert (E.CASES[n]['sigma'], E.CASES[n]['width']) == (2, 1.5)


@pytest.mark.parametrize('name', E.NAMES)
def test_visible_coordinates_are_finite_and_sizes_are_multiples_of_8(name):
    c = E.CASES[name]
    p = c['poses']
    assert p.dtype == np.float64 and p.shape[1:] == (18, 3)
    assert np.isfinite(p[p[:, :, 2] > 0][:, :2]).all()
    assert c['hw'][0] % 8 == 0 and c['hw'][1] % 8 == 0 and c['sigma'] > 0 and c['width'] >= 0


@pytest.mark.parametrize('name', [n for n in E.NAMES if n not in E.INTEGER_AXES])
def test_no_pixel_sits_on_a_band_edge(name):
    c = E.CASES[name]
    _, margin = E.bands(c['hw'], c['poses'], c['width'])
    print(name, 'band margin %.3g' % margin)
    assert margin > 1e-9


def test_outside4_has_a_visible_joint_beyond_each_side_and_a_limb_across_a_border():
    c = E.CASES['outside4']
    (h, w), p = c['hw'], c['poses']
    vis = p[p[:, :, 2] > 0]
    assert (vis[:, 0] < 0).any() and (vis[:, 0] > w - 1).any() and (vis[:, 1] < 0).any() and (vis[:, 1] > h - 1).any()
    inside = (p[:, :, 0] >= 0) & (p[:, :, 0] <= w - 1) & (p[:, :, 1] >= 0) & (p[:, :, 1] <= h - 1)
    assert any(q[ja, 2] > 0 and q[jb, 2] > 0 and i[ja] != i[jb] for q, i in zip(p, inside) for ja, jb in LIMBS_POINT)


def test_far_is_all_zero_with_background_one(lab):
    paf, heat = lab['far']
    assert not paf.any() and not heat[:18].any() and (heat[18] == 1).all()
    assert E.CASES['far']['poses'][:, :, 0].min() > 300


def test_parallel2_and_cross_have_pixels_under_two_bands(lab):
    c = E.CASES['parallel2']
    cover, _ = E.bands(c['hw'], c['poses'], c['width'])
    assert set(np.unique(cover)) == {0, 2}
    one = loss_ref.labels(c['hw'], c['poses'][:1], c['sigma'], c['width'])
    assert np.array_equal(lab['parallel2'][0], one[0]) and np.array_equal(lab['parallel2'][1], one[1])     # (u + u) / 2 == u
    c = E.CASES['cross']
    cover, _ = E.bands(c['hw'], c['poses'], c['width'])
    assert (cover[0] == 2).sum() >= 4          # limb 0, turned about its own midpoint
    ua, ub = (q[E.RHIP, :2] - q[E.NECK, :2] for q in c['poses'])
    cos = ua @ ub / np.linalg.norm(ua) / np.linalg.norm(ub)
    assert abs(np.degrees(np.arccos(cos)) - 60) < 1e-9
    # under both bands the value is the mean of the two unit vectors: shorter than either
    paf = lab['cross'][0]
    both = cover[0] == 2
    norm = np.hypot(paf[0], paf[1])
    assert np.allclose(norm[both], np.cos(np.pi / 6), atol=1e-6) and np.allclose(norm[cover[0] == 1], 1, atol=1e-6)


def test_anti_cancels_to_exact_zero_under_both_bands(lab):
    c = E.CASES['anti']
    a, b = c['poses']
    assert np.array_equal(a[E.NECK], b[E.RHIP]) and np.array_equal(a[E.RHIP], b[E.NECK])
    both = (E.bands(c['hw'], a[None], c['width'])[0][0] == 1) & (E.bands(c['hw'], b[None], c['width'])[0][0] == 1)
    assert both.sum() >= 20
    paf = lab['anti'][0]
    assert not paf[0][both].any() and not paf[1][both].any()
    alone = loss_ref.labels(c['hw'], a[None], c['sigma'], c['width'])[0]
    assert alone[0][both].all() and alone[1][both].all()          # ... where one person alone has a non-zero vector


def test_width0_sets_between_one_pixel_and_a_segment_per_limb():
    c = E.CASES['width0']
    h, w = c['hw']
    for q in c['poses']:
        assert (q[:, 0] == np.round(q[:, 0])).all() and (q[:, 1] == np.round(q[:, 1])).all()
        assert (q[:, 0] >= 0).all() and (q[:, 0] <= w - 1).all() and (q[:, 1] >= 0).all() and (q[:, 1] <= h - 1).all()
        paf = loss_ref.labels(c['hw'], q[None], c['sigma'], 0.0)[0]
        for li, (ja, jb) in enumerate(LIMBS_POINT):
            nz = (paf[2 * li] != 0) | (paf[2 * li + 1] != 0)
            assert 1 <= nz.sum() <= 2 * max(h, w), (li, nz.sum())
            # only pixels on the segment
            ys, xs = np.nonzero(nz)
            for x, y in zip(xs, ys):
                assert min(q[ja, 0], q[jb, 0]) <= x <= max(q[ja, 0], q[jb, 0]) and min(q[ja, 1], q[jb, 1]) <= y <= max(q[ja, 1], q[jb, 1])


def test_special_joints_are_what_the_cases_say():
    p = E.CASES['coincident_v1']['poses']
    assert (p[:, :, 2] == 1).all() and np.array_equal(p[0, 3, :2], p[0, 4, :2]) and p[0, 3, 0] != np.round(p[0, 3, 0])
    p = E.CASES['invisible_between']['poses']
    assert (p[1, :, 2] == 0).all() and (p[0, :, 2] > 0).all() and (p[2, :, 2] > 0).all()
    assert p[0, 0, 0] < p[1, 0, 0] < p[2, 0, 0]
    c = E.CASES['invisible_between']
    q = p.copy()
    q[1, :, 2] = 2
    seen = loss_ref.labels(c['hw'], q, c['sigma'], c['width'])
    shown = loss_ref.labels(c['hw'], p, c['sigma'], c['width'])
    assert not np.array_equal(seen[0], shown[0]) and not np.array_equal(seen[1], shown[1])       # a visible middle person would show
    p = E.CASES['tiny_limb']['poses'][0]
    assert abs(np.linalg.norm(p[3, :2] - p[2, :2]) - 1e-3) < 1e-12
    c = E.CASES['tiny_limb']
    paf = loss_ref.labels(c['hw'], c['poses'], c['sigma'], c['width'])[0]
    limb = [tuple(l) for l in LIMBS_POINT].index((2, 3))
    assert (paf[2 * limb] != 0).sum() == 1 and paf[2 * limb][9, 12] != 0
    p = E.CASES['crowd24']['poses']
    assert set(np.unique(p[:, :, 2])) == {0, 1, 2}
    for n in ('row8', 'col8', 'one8'):
        c = E.CASES[n]
        paf = loss_ref.labels(c['hw'], c['poses'], c['sigma'], c['width'])[0]
        assert paf.any(), n


@pytest.mark.skipif(not R.reference_available(), reason='the reference is not present')
@pytest.mark.parametrize('name', E.NAMES)
def test_loss_ref_labels_equal_the_live_reference(lab, name):
    c = E.CASES[name]
    _, _, _, gen = R.import_reference()
    img = np.zeros(c['hw'] + (3,), np.uint8)
    heat = gen.generate_heatmaps(img, c['poses'], c['sigma'])
    paf = gen.generate_pafs(img, c['poses'], c['width'])
    assert heat.dtype == np.float32 and paf.dtype == np.float32
    assert np.array_equal(paf, lab[name][0]) and np.array_equal(heat, lab[name][1])


def test_targets_of_one_map_pixel_are_label_pixel_00(lab):
    paf, heat = lab['one8']
    t_p, t_h, t_m = loss_ref.targets(paf, heat, None)
    assert t_p.shape == (38, 1, 1) and np.array_equal(t_p[:, 0, 0], paf[:, 0, 0]) and np.array_equal(t_h[:, 0, 0], heat[:, 0, 0])
    assert heat[:18, 0, 0].any() and not t_m.any()
    mask = np.zeros((8, 8), bool)
    mask[0, 1] = mask[1, 0] = mask[7, 7] = True              # every pixel but (0, 0) has weight 0
    assert not loss_ref.targets(paf, heat, mask)[2].any()
    mask[0, 0] = True
    assert loss_ref.targets(paf, heat, mask)[2].all()
    # 8 x 8 crops of the strips give the same
    for n in ('row8', 'col8'):
        t = loss_ref.targets(lab[n][0][:, :8, :8], lab[n][1][:, :8, :8], None)
        assert np.array_equal(t[0][:, 0, 0], lab[n][0][:, 0, 0]) and np.array_equal(t[1][:, 0, 0], lab[n][1][:, 0, 0])


@pytest.mark.parametrize('name', ['row8', 'col8'])
def test_targets_of_a_strip_are_the_corner_aligned_line(lab, name):
    """8 x 40 -> 1 x 5: row 0 of the labels at the columns k * 39 / 4, the two neighbours weighted in float32; 40 x 8 likewise in y"""
    h, w = E.CASES[name]['hw']
    t_p, t_h, _ = loss_ref.targets(lab[name][0], lab[name][1], None)
    for t, full in ((t_p, lab[name][0]), (t_h, lab[name][1])):
        line = full[:, 0, :] if name == 'row8' else full[:, :, 0]
        n = line.shape[1]
        assert t.shape[1:] == ((1, 5) if name == 'row8' else (5, 1))
        got = t[:, 0, :] if name == 'row8' else t[:, :, 0]
        for k in range(5):
            u = k * (n - 1) / 4.0
            i0 = int(np.floor(u))
            i1 = min(i0 + 1, n - 1)
            lo, hi = np.float32(i0 + 1 - u), np.float32(u - i0)
            want = lo * line[:, i0] + hi * line[:, i1]
            assert want.dtype == np.float32 and np.array_equal(got[:, k], want), (name, k)
        assert np.array_equal(got[:, 0], line[:, 0]) and np.array_equal(got[:, 4], line[:, n - 1])
        assert got.any()
