"""The pair-walk forward kernel (lasr_amd/csrc/sr_forward_pairs.h) DEALS a tile's face list round-robin over its chunks: a round of
`count` entries makes nch = ceil(count / 64) chunks, chunk c holds the list positions c, c + nch, c + 2 nch, ... (chunk_count,
chunk_size, chunk_pos in the header; tests/test_pair_walk_chunk_deal_cases.py restates them).  Chunks are then partial whenever
count is no multiple of 64 -- 65 entries are 33 + 32 -- so lanes ride along on slot 63 of a staging buffer that no chunk of the
workgroup has written, and a pixel meets its fragments residue class by residue class.  Which chunk an entry lands in must not
show beyond rounding.

Scenes, the smallest shapes at which the deal can go wrong: one 16x16 tile under K stacked triangles at distinct depths, K = 65
(33 + 32: every chunk partial, the workgroup's first included), 128 (64 + 64: the slot is staged), 129 (three chunks of 43) and 130
(44 + 43 + 43: a remainder); a crowded mesh at 16, 20 and 33 pixels (ragged tiles); tame and non-tame records in one chunk (the slow
mask's bits follow their lane's entry); six and nine channels; three frames at 64; eight frames at 64 (the smallest launch that
issues its tiles in an order of its own); 2500 faces in the centre of a 64x64 image (more than one list round; held to 1e-5 as in
tests/test_forward_kernel_choice_gpu.py).

Every scene is forced through the pair walk, with one team and with two teams of four waves per tile (team t walks the chunks
t, t + 2, ...: with an odd chunk count one team makes a trip with no entries), and held against the CPU oracle (colours <= 1e-6,
the project's PAIR_TOL), against the one-wave reference-order kernel (the running-maximum plane aggrs[:, 1] exactly), against a
second run (bit-equal), in the fixed tile order against the launch's own (bit-equal), and one team against two (<= PAIR_TOL)."""
import numpy as np
import pytest

import raster_harness as rh
from lasr_amd import _lib, synth
from lasr_amd.soft_renderer import functional as srf
from raster_harness import ONE_WAVE, PAIR_TOL, PAIR_WALK, PAIR_WALK_FIXED, PAIR_WALK_OWN, same_bits, stack


def _channels(C):
    fv, ft, near, far = synth.raster_batch(4, 3, count=2)
    return fv, rh.more_channels(ft, C, np.random.default_rng(C)), near, far


# name -> (scene builder, image size, colour tolerance against the oracle); every scene is (face_vertices, textures, near, far)
CASES = {
    'stack of 65': (lambda: stack(65), 16, PAIR_TOL),
    'stack of 128': (lambda: stack(128), 16, PAIR_TOL),
    'stack of 129': (lambda: stack(129), 16, PAIR_TOL),
    'stack of 130': (lambda: stack(130), 16, PAIR_TOL),
    'crowded 16': (lambda: synth.raster_batch(4, 3, count=1), 16, PAIR_TOL),
    'ragged 20': (lambda: synth.raster_batch(4, 3, count=1), 20, PAIR_TOL),
    'ragged 33': (lambda: synth.raster_batch(4, 3, count=1), 33, PAIR_TOL),
    'tame and not tame': (rh.not_tame, 64, PAIR_TOL),
    'six channels': (lambda: _channels(6), 48, PAIR_TOL),
    'nine channels': (lambda: _channels(9), 48, PAIR_TOL),
    'three frames': (lambda: synth.raster_batch(4, 3, count=3), 64, PAIR_TOL),
    'eight frames': (lambda: synth.raster_batch(4, 5, count=8), 64, PAIR_TOL),
    'long list': (rh.long_list, 64, 1e-5),      # tests/test_forward_kernel_choice_gpu.py holds it to 1e-5 as well
}


def background(C):
    return [1., 1., 1.] if C == 3 else [0.25 * k for k in range(C)]


def oracle_image(oracle, name):
    """The oracle's image of a case, [N, C + 1, IS, IS] (alpha last); computed once."""
    def compute():
        fv, ft, near, far = CASES[name][0]()
        return rh.oracle_reference(oracle, fv, ft, CASES[name][1], background(ft.shape[-1]), dict(synth.LASR_MODES, near=near, far=far))[0]
    return rh.cached(('chunk deal', name), compute)


def render(dev, scene, IS):
    """(soft_colors, aggrs_info) of a scene through the operator's forward, with the launch options and flags in force."""
    return rh.render(dev, scene, IS, background(scene[1].shape[-1]))


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_dealt_chunks_agree_with_the_oracle_and_keep_the_running_maximum(oracle, cuda, name):
    build, IS, tol = CASES[name]
    scene = build()
    ref = oracle_image(oracle, name)
    out = {}
    try:
        srf.set_launch_thresholds(*ONE_WAVE)
        _, aggr_ref = render(cuda, scene, IS)
        for flag, teams in ((_lib.SR_PAIR_ONE_TEAM, 'one team'), (_lib.SR_PAIR_TWO_TEAMS, 'two teams')):
            srf.set_forward_flags(flag)
            srf.set_launch_thresholds(*PAIR_WALK)
            img, aggr = render(cuda, scene, IS)
            img2, aggr2 = render(cuda, scene, IS)
            srf.set_launch_thresholds(*PAIR_WALK_FIXED)
            img_f, aggr_f = render(cuda, scene, IS)
            srf.set_launch_thresholds(*PAIR_WALK_OWN)
            img_o, aggr_o = render(cuda, scene, IS)
            err = float(np.abs(img - ref).max())
            print('%s, %s: pair walk against the oracle, max abs %.3e' % (name, teams, err))
            assert img.shape == ref.shape and np.isfinite(img).all()
            assert err <= tol, '%s, %s: max %.3e' % (name, teams, err)
            assert np.array_equal(aggr[:, 1], aggr_ref[:, 1]), '%s, %s: running maximum differs from the one-wave kernel' % (name, teams)
            assert same_bits(img, img2) and same_bits(aggr, aggr2), '%s, %s: a second run differs' % (name, teams)
            assert same_bits(img_f, img_o) and same_bits(aggr_f, aggr_o), '%s, %s: the tile order shows' % (name, teams)
            assert same_bits(img, img_f) and same_bits(aggr, aggr_f)
            out[teams] = img
    finally:
        srf.set_forward_flags(_lib.SR_DEFAULT_FLAGS)
        srf.set_launch_thresholds()
    d = float(np.abs(out['one team'] - out['two teams']).max())
    print('%s: one team against two, max abs %.3e' % (name, d))
    assert d <= PAIR_TOL, '%s: one team against two, max %.3e' % (name, d)
