"""The pair-walk forward kernel (lasr_amd/csrc/sr_forward_pairs.h) evens out its two per-lane loops inside a wave: before the
classification loop the lanes are ranked by their candidate count and rank r is partnered with rank 63 - r; the lighter lane takes
the upper half of the difference, classifies those bits at the HEAVIER lane's pixel centre and hands the two result masks back.
The walk does the same with outside pairs.  Which lane evaluates a bit must not show: every case below is forced through the pair
walk and held against the CPU oracle (colours <= 1e-6, the project's PAIR_TOL), against the one-wave reference-order kernel (the
running-maximum plane aggrs[:, 1] exactly), and against a second run (bit-equal).

The cases are the smallest shapes at which the hand-off can go wrong: one crowded 16x16 tile with several chunks; ragged images
(lanes outside the image are light partners and classify at coordinates that are not theirs); 70 stacked triangles over the left
half of a tile (64 candidates against none: the largest transfer, all inside pairs, which the walk must not move); the same stack
shrunk to a sliver beside one pixel column (all outside-but-near: the walk moves the maximum); one face, no face; tame and
non-tame records in one chunk (slow-mask bits stay with their lane); six and nine channels; one and two teams per tile.
tests/test_pair_walk_lane_balance_cases.py checks on the CPU that these scenes are not background only."""
import numpy as np
import pytest

import raster_harness as rh
from lasr_amd import _lib, synth
from lasr_amd.soft_renderer import functional as srf
from raster_harness import ONE_WAVE, PAIR_TOL, PAIR_WALK


def _stack(shrunk):
    """70 identical triangles at distinct depths in one 16x16 image.  Whole: the vertical edge at x = -0.03 puts the pixel centres
    of columns 0..7 inside and leaves columns 8..15 outside the faces' pixel rect (threshold radius 0.0304).  Shrunk: a sliver
    0.0275 left of column 7's centres (x = -0.0625) and 0.0775 right of column 6's: column 7 is outside but near, nothing else is."""
    fv, ft, near, far = rh.stack(70)
    if shrunk:
        fv[0, :, :, :2] = np.asarray([[-0.09, -0.9], [-0.09, 0.9], [-0.11, 0.]], np.float32)
    return fv, ft, near, far


def _channels(C):
    fv, ft, near, far = synth.raster_batch(4, 3, count=2)
    return fv, rh.more_channels(ft, C, np.random.default_rng(C)), near, far


def _one_face():
    fv = np.array([[[[-0.4, -0.3, 3.], [0.5, -0.2, 3.5], [0.1, 0.6, 2.5]]]], np.float32)
    return fv, np.array([[[[1., 0., 0.], [0., 1., 0.], [0., 0., 1.]]]], np.float32), 1.0, 5.0


def _empty():
    e = np.zeros((1, 0, 3, 3), np.float32)
    return e, e.copy(), 1.0, 5.0


# name -> (scene builder, image size); every scene is (face_vertices, textures, near, far)
CASES = {
    'one crowded tile': (lambda: synth.raster_batch(4, 3, count=1), 16),
    'ragged 20': (lambda: synth.raster_batch(4, 3, count=1), 20),
    'ragged 33': (lambda: synth.raster_batch(4, 3, count=1), 33),
    'stack over the left half': (lambda: _stack(False), 16),
    'stack shrunk to a sliver': (lambda: _stack(True), 16),
    'one face': (_one_face, 16),
    'empty mesh': (_empty, 16),
    'tame and not tame': (rh.not_tame, 64),
    'six channels': (lambda: _channels(6), 48),
    'nine channels': (lambda: _channels(9), 48),
    'three frames': (lambda: synth.raster_batch(4, 3, count=3), 64),
}


def background(C):
    return [1., 1., 1.] if C == 3 else [0.25 * k for k in range(C)]


def oracle_image(oracle, name):
    """The oracle's image of a case, [N, C + 1, IS, IS] (alpha last); computed once."""
    def compute():
        fv, ft, near, far = CASES[name][0]()
        return rh.oracle_reference(oracle, fv, ft, CASES[name][1], background(ft.shape[-1]), dict(synth.LASR_MODES, near=near, far=far))[0]
    return rh.cached(('lane balance', name), compute)


def render(dev, name):
    """(soft_colors, aggrs_info) of a case through the operator's forward, with the launch options and flags in force."""
    build, IS = CASES[name]
    scene = build()
    return rh.render(dev, scene, IS, background(scene[1].shape[-1]))


@pytest.fixture
def launch():
    yield srf.set_launch_thresholds
    srf.set_forward_flags(_lib.SR_DEFAULT_FLAGS)
    srf.set_launch_thresholds()


def check(oracle, dev, launch, name):
    ref = oracle_image(oracle, name)
    launch(*ONE_WAVE)
    _, aggr_ref = render(dev, name)
    launch(*PAIR_WALK)
    img, aggr = render(dev, name)
    img2, aggr2 = render(dev, name)
    err = float(np.abs(img - ref).max()) if ref.size else 0.
    print('%s: pair walk against the oracle, max abs %.3e' % (name, err))
    assert img.shape == ref.shape and np.isfinite(img).all()
    assert err <= PAIR_TOL, '%s: max %.3e' % (name, err)
    assert np.array_equal(aggr[:, 1], aggr_ref[:, 1]), name + ': running maximum differs from the one-wave kernel'
    assert np.array_equal(img.view(np.uint32), img2.view(np.uint32)) and np.array_equal(aggr.view(np.uint32), aggr2.view(np.uint32))
    return img


@pytest.mark.gpu
@pytest.mark.parametrize('name', [n for n in CASES if n != 'three frames'])
def test_the_balanced_pair_walk_agrees_with_the_oracle_and_keeps_the_running_maximum(oracle, cuda, launch, name):
    img = check(oracle, cuda, launch, name)
    if name == 'empty mesh':
        assert np.array_equal(img[:, :3], np.ones_like(img[:, :3])) and not img[:, 3].any()


@pytest.mark.gpu
def test_one_and_two_teams_agree_with_the_oracle_and_each_other(oracle, cuda, launch):
    out = {}
    for flag in (_lib.SR_PAIR_ONE_TEAM, _lib.SR_PAIR_TWO_TEAMS):
        srf.set_forward_flags(flag)
        out[flag] = check(oracle, cuda, launch, 'three frames')
    d = float(np.abs(out[_lib.SR_PAIR_ONE_TEAM] - out[_lib.SR_PAIR_TWO_TEAMS]).max())
    print('one team against two: max abs %.3e' % d)
    assert d <= PAIR_TOL
