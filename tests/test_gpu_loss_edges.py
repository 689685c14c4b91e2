"""GPU: the label kernels of csrc/pmx_loss.hip (loss_labels_kernel: every pixel; loss_targets_kernel: the corner pixels of the map) on the
case table tests/loss_edge_cases.py against the NumPy restatement tests/loss_ref.py, which tests/test_loss_edges_host.py pins to the
verbatim reference on the same cases.  Bounds: the device's and glibc's float64 exp may differ in the last bit before the float32 cast,
so a value may move by one float32 ulp of 1 (2**-23, the bound of tests/test_gpu_validation_loss.py); which pixels a band holds is
demanded exactly (no pixel of a case lies within 1e-9 of a band edge: host file), and the two device paths to the targets are compared
with each other at zero tolerance."""
import numpy as np
import pytest

import loss_edge_cases as E
import loss_ref

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
MASKS = ('none', 'dense', 'sparse')


def mask_of(kind, h, w, seed=0):
    """None, about 60 % set, or about 1 % set (at least one pixel); seeded"""
    if kind == 'none':
        return None
    rng = np.random.default_rng(7100 + seed)
    if kind == 'dense':
        return rng.uniform(size=(h, w)) < 0.6
    m = np.zeros(h * w, bool)
    m[rng.choice(h * w, max(1, round(0.01 * h * w)), replace=False)] = True
    return m.reshape(h, w)


@pytest.fixture(scope='module')
def ref():
    """loss_ref.labels of every case: computed once, never modified"""
    return {n: loss_ref.labels(c['hw'], c['poses'], c['sigma'], c['width']) for n, c in E.CASES.items()}


@pytest.fixture(scope='module')
def engines(native):
    """one context per image size of the table, sized to it (batch 4 for the placement test)"""
    made = {}

    def get(hw, batch=1):
        if (hw, batch) not in made:
            made[hw, batch] = native.Engine(0, max_batch=batch, max_h=hw[0], max_w=hw[1])
        return made[hw, batch]
    yield get
    for e in made.values():
        e.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


@pytest.mark.parametrize('name', E.NAMES)
def test_labels_of_every_pixel(engines, ref, name):
    c = E.CASES[name]
    h, w = c['hw']
    e = engines(c['hw'])
    e.loss_set_poses([c['poses']], h, w, None, c['sigma'], c['width'])
    paf, heat = e.labels(0)
    want_p, want_h = ref[name]
    dp, dh = np.abs(paf - want_p).max(), np.abs(heat - want_h).max()
    print(name, 'labels: paf %.3g heat %.3g ulp' % (dp / ULP, dh / ULP))
    assert np.array_equal(paf != 0, want_p != 0)
    assert dp <= ULP and dh <= ULP
    if name in ('anti', 'far', 'width0'):
        assert not _bits(paf)[want_p == 0].any()          # +0.0f, not a small number and not -0.0f
    if name == 'far':
        assert not _bits(heat[:18]).any() and (heat[18] == 1).all()
    if name == 'anti':
        both = (E.bands(c['hw'], c['poses'][:1], c['width'])[0][0] == 1) & (E.bands(c['hw'], c['poses'][1:], c['width'])[0][0] == 1)
        assert both.any() and not _bits(paf[:2])[:, both].any()


@pytest.mark.parametrize('name', E.NAMES)
def test_targets_from_poses_and_from_the_devices_own_labels(engines, ref, name):
    c = E.CASES[name]
    h, w = c['hw']
    e = engines(c['hw'])
    for i, kind in enumerate(MASKS):
        mask = mask_of(kind, h, w, i)
        m1 = None if mask is None else mask[None]
        want_p, want_h, want_m = loss_ref.targets(ref[name][0], ref[name][1], mask)
        e.loss_set_poses([c['poses']], h, w, m1, c['sigma'], c['width'])          # form (b): only the corner pixels
        paf_t, heat_t, mask_t = e.loss_targets()
        dp, dh = np.abs(paf_t[0] - want_p).max(), np.abs(heat_t[0] - want_h).max()
        print(name, kind, 'targets: paf %.3g heat %.3g ulp' % (dp / ULP, dh / ULP))
        assert dp <= ULP and dh <= ULP
        assert np.array_equal(mask_t[0], want_m)
        assert np.array_equal(paf_t[0] != 0, want_p != 0)
        # form (a) fed back at full size: the same float32 combine4 of the same float64 label values, so the same bytes
        paf, heat = e.labels(0)
        e.loss_set_targets(paf[None], heat[None], h, w, m1)
        paf_r, heat_r, mask_r = e.loss_targets()
        assert np.array_equal(_bits(paf_r), _bits(paf_t)) and np.array_equal(_bits(heat_r), _bits(heat_t))
        assert np.array_equal(mask_r, mask_t)
        if kind == 'dense' and c['hw'] == E.HW:
            assert want_m.any() and not want_m.all()


PLACEMENT = ('empty', 'invisible_between', 'empty', 'crowd24')          # people counts (0, 3, 0, 24): off[] stands, steps, stands, steps


def _placement_inputs(order):
    h, w = E.HW
    poses = [np.zeros((0, 18, 3)) if PLACEMENT[i] == 'empty' else E.CASES[PLACEMENT[i]]['poses'] for i in order]
    masks = np.stack([np.zeros((h, w), bool) if i == 0 else mask_of(('dense', 'sparse', 'dense')[i - 1], h, w, 10 + i) for i in order])
    return poses, masks


def test_batch_placement(engines, ref):
    """one call with four images = four calls with one = the same batch in reversed order, byte for byte"""
    h, w = E.HW
    e = engines(E.HW, 4)
    poses, masks = _placement_inputs(range(4))
    assert [len(p) for p in poses] == [0, 3, 0, 24]
    e.loss_set_poses(poses, h, w, masks, E.SIGMA, E.WIDTH)
    paf_t, heat_t, mask_t = e.loss_targets()
    labels4 = [e.labels(i) for i in range(4)]
    for i in range(4):
        e.loss_set_poses(poses[i:i + 1], h, w, masks[i:i + 1], E.SIGMA, E.WIDTH)
        p1, h1, m1 = e.loss_targets()
        assert np.array_equal(_bits(p1[0]), _bits(paf_t[i])) and np.array_equal(_bits(h1[0]), _bits(heat_t[i])), i
        assert np.array_equal(m1[0], mask_t[i]), i
        l1 = e.labels(0)
        assert np.array_equal(_bits(l1[0]), _bits(labels4[i][0])) and np.array_equal(_bits(l1[1]), _bits(labels4[i][1])), i
        # and against the restatement
        if PLACEMENT[i] == 'empty':
            assert not paf_t[i].any() and not heat_t[i][:18].any() and (heat_t[i][18] == 1).all()
        else:
            want = loss_ref.targets(ref[PLACEMENT[i]][0], ref[PLACEMENT[i]][1], masks[i])
            assert np.abs(paf_t[i] - want[0]).max() <= ULP and np.abs(heat_t[i] - want[1]).max() <= ULP
            assert np.array_equal(mask_t[i], want[2])
    assert paf_t[1].any() and paf_t[3].any() and not np.array_equal(paf_t[1], paf_t[3])
    rposes, rmasks = _placement_inputs(range(3, -1, -1))
    assert [len(p) for p in rposes] == [24, 0, 3, 0]
    e.loss_set_poses(rposes, h, w, rmasks, E.SIGMA, E.WIDTH)
    p_r, h_r, m_r = e.loss_targets()
    assert np.array_equal(_bits(p_r[::-1]), _bits(paf_t)) and np.array_equal(_bits(h_r[::-1]), _bits(heat_t))
    assert np.array_equal(m_r[::-1], mask_t)
    for i in range(4):
        lr = e.labels(3 - i)
        assert np.array_equal(_bits(lr[0]), _bits(labels4[i][0])) and np.array_equal(_bits(lr[1]), _bits(labels4[i][1])), i
