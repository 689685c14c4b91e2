"""Host side of the device renderer (include/pose_mi355x.h::pmx_render, native.Engine.render, PoseDetector.draw_batch,
demo.render_batch): what the header and the build declare, the argument checks that run before the device is touched, the CLI flags."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import pkg


def test_header_declares_the_entry_and_states_the_contract():
    native = pkg('native')
    assert 'pmx_render' in native.header_symbols()
    txt = open(native.HEADER).read()
    m = re.search(r'typedef struct pmx_render_part \{([^}]*)\} pmx_render_part;', txt)
    assert m, 'pmx_render_part is not declared'
    fields = [f.strip() for f in re.sub(r'/\*.*?\*/', '', m.group(1)).replace('int ', '').rstrip('; ').split(',')]
    assert fields == [name for name, _ in native.PmxRenderPart._fields_]
    assert all(t is C.c_int for _, t in native.PmxRenderPart._fields_)
    # the contract is written out: the host functions it restates and the three arithmetic rules
    for word in ('draw_person_pose', 'add_weighted', 'draw_face_keypoints', 'draw_hand_keypoints', 'draw_rectangle', '_draw_line',
                 '_draw_disc', 'r * r + 0.25', 'half to even', 'img * 0.6f + c * 0.4f + 0.0f', 'LAST'):
        assert word in txt, word


def test_the_unit_is_built_without_contraction():
    native = pkg('native')
    assert ('pmx_render.hip', ['-ffp-contract=off']) in native.SOURCES


def test_binding_carries_the_signature(native):
    lib = native.load()
    assert 'pmx_render' in lib._pmx_sig and len(lib._pmx_sig['pmx_render'][1]) == 12
    assert hasattr(lib, 'pmx_render')


def _img(h=8, w=9):
    return np.zeros((h, w, 3), np.uint8)


FACE = ('face', (1, 2, 30, 40), [[1.5, 2.25, 0.5]] * 69 + [None])
HAND = ('hand', (-3, 2, 10, 12), [None] + [[2, 3, np.float32(0.25)]] * 20)


def test_render_args_flatten():
    native = pkg('native')
    poses = [np.zeros((0, 18, 3)), np.arange(108.0).reshape(2, 18, 3), []]
    p, n, parts, n_parts, kps = native.render_args([_img(), _img(), _img(4, 4)], poses, [[], [FACE, HAND], [HAND]])
    assert p.shape == (2, 18, 3) and p.dtype == np.float64 and n.tolist() == [0, 2, 0] and n.dtype == np.int32
    assert n_parts == 3 and kps.shape == (70 + 21 + 21, 4) and kps.dtype == np.float64
    assert [(q.image, q.kind, q.left, q.top, q.right, q.bottom) for q in parts[:3]] == [(1, 0, 1, 2, 30, 40), (1, 1, -3, 2, 10, 12), (2, 1, -3, 2, 10, 12)]
    assert kps[0].tolist() == [1.5, 2.25, 0.5, 1.0] and kps[69].tolist() == [0, 0, 0, 0]
    assert kps[70].tolist() == [0, 0, 0, 0] and kps[71].tolist() == [2, 3, 0.25, 1.0]
    # nothing to draw is fine; rows (x, y, confidence, valid) are taken as they are
    p, n, parts, n_parts, kps = native.render_args([], [], None)
    assert len(p) == 0 and len(n) == 0 and n_parts == 0 and len(kps) == 0
    rows = np.zeros((21, 4)); rows[3] = (1, 2, 0.5, 1)
    assert native.render_args([_img()], [[]], [[('hand', (0, 0, 5, 5), rows)]])[4][3].tolist() == [1, 2, 0.5, 1]


BAD_ARGS = [
    ('poses per image', lambda: ([_img(), _img()], [[]], None, True)),
    ('parts per image', lambda: ([_img()], [[]], [[], []], True)),
    ('float image', lambda: ([np.zeros((8, 9, 3), np.float32)], [[]], None, True)),
    ('grey image', lambda: ([np.zeros((8, 9), np.uint8)], [[]], None, True)),
    ('four channels', lambda: ([np.zeros((8, 9, 4), np.uint8)], [[]], None, True)),
    ('empty image', lambda: ([np.zeros((0, 9, 3), np.uint8)], [[]], None, True)),
    ('not an image', lambda: ([[[1, 2, 3]]], [[]], None, True)),
    ('poses (n, 17, 3)', lambda: ([_img()], [np.zeros((1, 17, 3))], None, True)),
    ('poses (18, 3)', lambda: ([_img()], [np.zeros((18, 3))], None, True)),
    ('unknown part', lambda: ([_img()], [[]], [[('foot', (0, 0, 1, 1), [None] * 21)]], True)),
    ('69 face points', lambda: ([_img()], [[]], [[('face', (0, 0, 1, 1), [None] * 69)]], True)),
    ('box of three', lambda: ([_img()], [[]], [[('hand', (0, 0, 1), [None] * 21)]], True)),
    ('box outside int32', lambda: ([_img()], [[]], [[('hand', (0, 0, 1, 2 ** 31), [None] * 21)]], True)),
    ('parts without blend', lambda: ([_img()], [[]], [[HAND]], False)),
]


@pytest.mark.parametrize('what,args', BAD_ARGS, ids=[w for w, _ in BAD_ARGS])
def test_argument_errors_raise_before_the_device(what, args):
    """The three Python forms on objects that have no context at all: a ValueError means nothing of the library was reached."""
    native, PD, demo = pkg('native'), pkg('pose_detector'), pkg('demo')
    imgs, poses, parts, blend = args()
    with pytest.raises(ValueError):
        native.render_args(imgs, poses, parts, blend)
    eng = object.__new__(native.Engine)
    with pytest.raises(ValueError):
        eng.render(imgs, poses, parts, blend)
    det = object.__new__(PD.PoseDetector)
    det.engine = eng
    if parts is None:
        with pytest.raises(ValueError):
            det.draw_batch(imgs, poses, blend)


def test_render_batch_checks_its_lists():
    native, PD, demo = pkg('native'), pkg('pose_detector'), pkg('demo')
    det = object.__new__(PD.PoseDetector)
    det.engine = object.__new__(native.Engine)
    person = {'unit_length': 10, 'face': None, 'left': {'bbox': (0, 0, 4, 4), 'keypoints': [None] * 20}, 'right': None}
    with pytest.raises(ValueError):
        demo.render_batch(det, [_img()], [[]], [])                       # one list of person parts per image
    with pytest.raises(ValueError):
        demo.render_batch(det, [_img()], [[]], [[person]])               # a hand of 20 key points
    with pytest.raises(ValueError):
        demo.render_batch(det, [_img()], [[], []], [[]])                 # one array of poses per image


def test_cli_flags_default_to_the_host():
    PD, demo = pkg('pose_detector'), pkg('demo')
    assert demo.parse_args(['--img', 'x.png']).render == 'host'
    assert demo.parse_args(['--img', 'x.png', '--render', 'device']).render == 'device'
    assert PD.parse_args(['posenet', 'w.npz', '--img', 'x.png']).render == 'host'
    a = PD.parse_args(['posenet', 'w.npz', '--img', 'x.png', '--render', 'device', '--gpu', '0'])
    assert (a.render, a.arch, a.weights, a.img, a.gpu, a.out, a.precise, a.precision) == ('device', 'posenet', 'w.npz', 'x.png', 0, 'result.png', False, 'f32')
    for mod, argv in ((demo, ['--img', 'x.png']), (PD, ['posenet', 'w.npz'])):
        with pytest.raises(SystemExit):
            mod.parse_args(argv + ['--render', 'opencv'])


def test_oracle_follows_the_formulas_of_the_header():
    """The host functions are the device form's oracle; here they are checked, on a few pixels each, against values worked out by hand
    from the formulas include/pose_mi355x.h writes out (segment within sqrt(r * r + 0.25), disc centre truncated toward zero, blend rounded
    half to even), so that header and oracle cannot drift apart unseen."""
    PD, demo = pkg('pose_detector'), pkg('demo')
    c = np.zeros((5, 7, 3), np.uint8)
    PD._draw_line(c, (1, 1), (5, 1), (9, 8, 7), 2)           # r = 1: rows 0..2 within sqrt(1.25) of the segment
    assert c[0, 3].tolist() == [9, 8, 7] and c[3, 3].tolist() == [0, 0, 0] and c[1, 0].tolist() == [9, 8, 7] and c[0, 0].tolist() == [0, 0, 0]
    d = np.zeros((9, 9, 3), np.uint8)
    PD._draw_disc(d, (4.9, -4.9), 5, (1, 2, 3))              # centre truncated toward zero: (4, -4)
    assert d[1, 4].tolist() == [1, 2, 3] and d[2, 4].tolist() == [0, 0, 0]
    assert demo.add_weighted(np.uint8([[[5]]]), 0.6, np.uint8([[[0]]]), 0.4)[0, 0, 0] == 3 and \
        demo.add_weighted(np.uint8([[[5]]]), 0.6, np.uint8([[[15]]]), 0.4)[0, 0, 0] == 9
