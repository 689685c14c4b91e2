"""CPU: csrc/pp_tables.h, the one layout and the one host-side builder of the post-process table sets, in a stand-alone program
(tests/pp_tables_dump.cpp, host compiler, no HIP): the bytes it writes equal oracle.postprocess_ref.resize_grid as float64 / int32
equality, the offsets it reports are the documented layout, the flipped grid is the reversed one, the taps block is zero behind the taps.
The program is built a second time with -fsanitize=address,undefined and that build runs the same cases once."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg
from oracle.postprocess_ref import resize_grid

# (in, out) of one axis: one pixel in, one pixel out (the num == 1 branch), down-sampling, the identity, the flagship's 46 <-> 368
AXES = [(1, 1), (1, 5), (5, 1), (4, 4), (3, 8), (46, 368), (368, 46), (7, 13)]
# every axis as the x axis with flip off and on ((7, 13) flipped among them), another axis as y: out_w != out_h in all but one case
GRIDS = [(AXES[(k + 3) % len(AXES)], AXES[k], flip) for k in range(len(AXES)) for flip in (0, 1)] + [((4, 4), (4, 4), 0)]
TAPS = [(21, 0, 0), (17, 1, 1), (1, 0, 0), (33, 0, 1)]
MAX_TAPS = 33                     # 2 * PMX_GAUSS_MAX_RADIUS + 1


def _args():
    a = []
    for (ih, oh), (iw, ow), flip in GRIDS:
        a += ['grid', ih, iw, oh, ow, flip]
    for t in TAPS:
        a += ['taps'] + list(t)
    return [str(v) for v in a]


def _build(tmp_path, name, extra):
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / name)
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-I', os.path.dirname(pkg('native').LIB_PATH)] + extra + \
          [os.path.join(ROOT, 'tests', 'pp_tables_dump.cpp'), '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(exe):
    r = subprocess.run([exe] + _args(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    out = _run(_build(tmp_path_factory.mktemp('pp_tables'), 'dump', []))
    recs = [json.loads(line) for line in out.splitlines()]
    assert len(recs) == len(GRIDS) + len(TAPS)
    return out, recs


def _arrays(rec):
    raw = bytes.fromhex(rec['raw'])
    assert len(raw) == rec['bytes']
    w, h = rec['out_w'], rec['out_h']
    a = {}
    for name, n, dt in (('xi0', w, np.int32), ('xi1', w, np.int32), ('yi0', h, np.int32), ('yi1', h, np.int32),
                        ('xlo', w, np.float64), ('xhi', w, np.float64), ('ylo', h, np.float64), ('yhi', h, np.float64)):
        a[name] = np.frombuffer(raw, dt, n, rec[name])
    return a


def test_sanitized_build_runs_clean_and_prints_the_same(tmp_path, dump):
    exe = _build(tmp_path, 'dump_san', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer'])
    assert _run(exe) == dump[0]


def test_grids_equal_the_oracle_exactly(dump):
    grids = [r for r in dump[1] if r['kind'] == 'grid']
    assert [((r['in_h'], r['out_h']), (r['in_w'], r['out_w']), r['flip']) for r in grids] == GRIDS
    for r in grids:
        a = _arrays(r)
        x, y = resize_grid(r['in_w'], r['out_w']), resize_grid(r['in_h'], r['out_h'])
        if r['flip']:
            x = [v[::-1] for v in x]
        for name, want in (('xi0', x[0]), ('xi1', x[1]), ('xlo', x[2]), ('xhi', x[3]), ('yi0', y[0]), ('yi1', y[1]), ('ylo', y[2]), ('yhi', y[3])):
            assert a[name].dtype == want.dtype and np.array_equal(a[name], want), (r['in_h'], r['in_w'], r['out_h'], r['out_w'], r['flip'], name)


def test_flipped_grid_is_the_reversed_unflipped_one(dump):
    grids = {(r['in_h'], r['in_w'], r['out_h'], r['out_w'], r['flip']): _arrays(r) for r in dump[1] if r['kind'] == 'grid'}
    pairs = 0
    for key, a in grids.items():
        if not key[4]:
            continue
        b = grids[key[:4] + (0,)]
        for name in ('xi0', 'xi1', 'xlo', 'xhi'):
            assert np.array_equal(a[name], b[name][::-1]), (key, name)
        for name in ('yi0', 'yi1', 'ylo', 'yhi'):
            assert np.array_equal(a[name], b[name]), (key, name)
        pairs += 1
    assert pairs == len(AXES) and any(k[1] == 7 and k[3] == 13 and k[4] for k in grids)


def test_layout_and_reported_size(dump):
    """[xi0 | xi1 | yi0 | yi1] ints from the block's first byte, padded to 8 bytes, then [xlo | xhi | ylo | yhi] doubles; the x arrays
    out_w long, the y arrays out_h long; the reported size ends with the last array"""
    for r in (r for r in dump[1] if r['kind'] == 'grid'):
        w, h = r['out_w'], r['out_h']
        assert (r['xi0'], r['xi1'], r['yi0'], r['yi1']) == (0, 4 * w, 8 * w, 8 * w + 4 * h)
        d0 = (8 * w + 8 * h + 7) // 8 * 8
        assert (r['xlo'], r['xhi'], r['ylo'], r['yhi']) == (d0, d0 + 8 * w, d0 + 16 * w, d0 + 16 * w + 8 * h)
        assert r['bytes'] == (r['yhi'] + 8 * h + 7) // 8 * 8
        # (the arrays tile the block: nothing of the 0xab fill is left where the ints end)
        assert bytes.fromhex(r['raw'])[r['yi1'] + 4 * h:r['xlo']] == b''


def test_taps_block_is_zero_behind_the_taps(dump):
    taps = [r for r in dump[1] if r['kind'] == 'taps']
    assert [(r['n'], r['border_zero'], r['nms_ge']) for r in taps] == TAPS
    for r in taps:
        assert r['bytes'] == MAX_TAPS * 8 and r['gauss'] == 0 and r['radius'] == (r['n'] - 1) // 2
        g = np.frombuffer(bytes.fromhex(r['raw']), np.float64)
        assert g.size == MAX_TAPS and np.array_equal(g[:r['n']], np.arange(1, r['n'] + 1, dtype=np.float64))
        assert not g[r['n']:].any() and not bytes.fromhex(r['raw'])[8 * r['n']:].strip(b'\0')
