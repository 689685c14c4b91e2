"""CPU: samples.draw_augmentation / transform_poses and the restatement's orchestration LIVE against the verbatim reference loader, where
the reference is present (tools/record_sample_goldens.py drives it); the recorded half of the same comparison is test_samples_host.py."""
import os
import random
import sys

import numpy as np
import pytest

import sample_ref
from conftest import ROOT, pkg
from oracle import _refimport as R

pytestmark = pytest.mark.skipif(not R.reference_available(), reason='the reference is not present')


@pytest.fixture(scope='module')
def tool():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import record_sample_goldens
    finally:
        sys.path.remove(os.path.join(ROOT, 'tools'))
    return record_sample_goldens


def test_draws_poses_and_samples_equal_the_live_reference(tool):
    S = pkg('samples')
    scenes = tool.make_inputs()
    for seed in range(100, 108):                       # seeds other than the recorded ones
        img, mask, poses = scenes[seed % len(scenes)]
        ref = tool.run_reference(img, mask, poses, seed)
        random.seed(seed)
        np.random.seed(seed)
        rec = S.draw_augmentation(img.shape[:2], poses, tool.INSIZE)
        d = rec.draws
        assert (d['u'], d['randn'], d['bbox_index'], d['r_xy']) == (ref['u'], ref['randn'], ref['index'], tuple(ref['r_xy']))
        assert rec.resized == tuple(ref['resized']) and rec.rotated == tuple(ref['rotated']) and np.array_equal(rec.R, ref['R'])
        assert (rec.distort is None) == (ref['distort'][0] == tool.MISSING) and (rec.distort is None or rec.distort == tuple(ref['distort']))
        assert rec.flip == bool(ref['flip'])
        assert np.array_equal(S.transform_poses(poses, rec), ref['poses'])
        got = sample_ref.prepare(img, mask, rec, tool.INSIZE)
        assert np.array_equal(got[0], ref['img']) and np.array_equal(got[2], ref['mask'])


def test_validation_sample_equals_the_live_reference(tool):
    S = pkg('samples')
    for img, mask, poses in tool.make_inputs():
        want_img, want_mask, want_poses = tool.run_reference_val(img, mask, poses)
        rec = S.SampleRecord.val(img.shape[:2], tool.INSIZE)
        got = sample_ref.prepare(img, mask, rec, tool.INSIZE)
        assert np.array_equal(got[0], want_img) and np.array_equal(got[2], want_mask)
        assert np.array_equal(S.transform_poses(poses, rec), want_poses)
