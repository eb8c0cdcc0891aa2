"""Every forward kernel form of the raster launcher's table (lasr_amd/csrc/sr_raster.hip: k_forward), at 3, 6 and 9 channels where it
exists, forced through the options and flags the other forward tests use -- and BEFORE each render lasr_sr_plan_forward, asked with
the same arguments, must name that form: the test knows which kernel ran instead of inferring it from the image.  The images are
held to the bars of test_forward_kernel_choice_gpu.py and test_forward_segmented_gpu.py: bit-equal to the one-wave kernel for
the forms that fold a pixel's fragments in the same order, within 1e-6 for the pair walk and the segmented forms; the relaxed
arithmetic and the generic kernel (another mode combination) within the north-star 1e-4 of the oracle, as test_raster_parity_gpu.py
holds them.  Shapes: 2 and 6 frames (6 frames of 64x64 are ordered: 384 tiles, from five frames) of 20x20 (ragged tiles at both
tile sizes) and 64x64 pixels.  For launches that leave the choice to the device, the plan's source and bound agree with the word
lasr_sr_peek_choice reads back."""
import numpy as np
import pytest

import raster_harness as rh
from lasr_amd import _lib, synth
from lasr_amd.soft_renderer import functional as srf
from raster_harness import BIG, PAIR_TOL

pytestmark = pytest.mark.gpu

IMG_TOL = 1e-4
NO_PAIRS = (-1, BIG)                    # order_max_tiles (default), pair_min_tiles
#  form: (options, flags, same bits as the one-wave kernel?)      `T` stands for the launch's 8x8 tile count
FORMS = {
    _lib.SR_FORM_ONE_WAVE: ((0, 0, 0) + NO_PAIRS, 0, True),
    _lib.SR_FORM_FOUR_WAVES: ((0, BIG, BIG) + NO_PAIRS, 0, True),
    _lib.SR_FORM_EIGHT_WAVES: ((BIG, BIG, BIG) + NO_PAIRS, 0, True),
    _lib.SR_FORM_SEG_FOUR: (('T-1', BIG, BIG) + NO_PAIRS, _lib.SR_SEGMENTED, False),     # above the eight-wave bound, below twice it
    _lib.SR_FORM_SEG_EIGHT: ((BIG, BIG, BIG) + NO_PAIRS, _lib.SR_SEGMENTED, False),
    _lib.SR_FORM_PAIRS_ONE_TEAM: ((0, 0, 0, -1, 0), _lib.SR_PAIR_ONE_TEAM, False),
    _lib.SR_FORM_PAIRS_TWO_TEAMS: ((0, 0, 0, -1, 0), _lib.SR_PAIR_TWO_TEAMS, False),
}


@pytest.fixture
def settings():
    def apply(options, flags):
        srf.set_launch_thresholds(*options)
        srf.set_forward_flags(flags)
    yield apply
    srf.set_forward_flags(_lib.SR_DEFAULT_FLAGS)
    srf.set_launch_thresholds()


def planned(N, F, IS, channels, options, flags, dist='euclidean'):
    return rh.plan(N, F, channels, IS, options, flags, rh.tail(dist_func=dist))


def render(dev, fv, ft, IS, kw):
    return rh.render(dev, (fv, ft), IS, want_aggrs=False, **kw)


def batch(N, channels):
    fv, ft, near, far = synth.raster_batch(4, 3, count=N)
    # attributes of the colours' magnitude: the 1e-6 bars are those of values in [0, 1]
    ft = rh.more_channels(ft, channels, np.random.default_rng(channels), -1, 1)
    kw = dict(synth.LASR_MODES, near=near, far=far, background_color=[0.125 * k for k in range(channels)])
    return fv, ft, kw


@pytest.mark.parametrize('channels', [3, 6, 9])
@pytest.mark.parametrize('N,IS', [(2, 20), (6, 20), (2, 64), (6, 64)])
def test_the_plan_names_the_kernel_that_renders_and_the_images_agree(settings, cuda, N, IS, channels):
    fv, ft, kw = batch(N, channels)
    F, tiles = fv.shape[1], N * ((IS + 7) // 8) ** 2
    want = None
    for form, (options, flags, same_bits) in FORMS.items():
        options = tuple(tiles - 1 if o == 'T-1' else o for o in options)
        p = planned(N, F, IS, channels, options, flags)
        assert p.form == form and p.both == 0, (form, p.form, p.both)
        side = 16 if form in (_lib.SR_FORM_PAIRS_ONE_TEAM, _lib.SR_FORM_PAIRS_TWO_TEAMS) else 8
        assert p.grid == N * ((IS + side - 1) // side) ** 2 and p.tile_shift == (4 if side == 16 else 3)
        assert p.ordered == (N >= 5 and (N * p.tso * p.tso) % 8 == 0)
        settings(options, flags)
        img = render(cuda, fv, ft, IS, kw)
        if want is None:
            want = img                                   # FORMS starts with the one-wave kernel
            assert img.shape == (N, channels + 1, IS, IS) and np.isfinite(img).all() and img[:, channels].max() > 0.5
        elif same_bits:
            assert np.array_equal(img.view(np.uint32), want.view(np.uint32)), (form, np.abs(img - want).max())
        else:
            err = np.abs(img - want).max()
            print('form %d, %d channels, %d x %d^2: max-abs %.3e against the one-wave kernel' % (form, channels, N, IS, err))
            assert err <= PAIR_TOL, (form, err)


@pytest.mark.parametrize('N,IS', [(2, 20), (6, 64)])
def test_relaxed_arithmetic_and_the_generic_kernel(settings, oracle, cuda, N, IS):
    fv, ft, kw = batch(N, 3)
    ref = oracle.forward(fv, ft, IS, **kw)['soft_colors']
    for channels in (3, 6, 9):                           # the relaxed one-wave kernel exists at every channel count
        fvc, ftc, kwc = batch(N, channels)
        for options in ((-1,) * 5, (BIG, BIG, BIG, -1, 0)):                 # whatever the thresholds say
            assert planned(N, fv.shape[1], IS, channels, options, _lib.SR_RELAXED_MATH).form == _lib.SR_FORM_ONE_WAVE_RELAXED
        settings((-1,) * 5, _lib.SR_RELAXED_MATH)
        img = render(cuda, fvc, ftc, IS, kwc)
        assert np.abs(img[:, :3] - ref[:, :3]).max() <= IMG_TOL and np.abs(img[:, channels] - ref[:, 3]).max() <= IMG_TOL
    # another mode combination (barycentric distance): the generic kernel, 256 threads per 16x16 tile, whatever the options and flags
    kwg = dict(kw, dist_func='barycentric')
    for options, flags in (((-1,) * 5, 0), ((BIG, BIG, BIG, BIG, 0), _lib.SR_SEGMENTED)):
        p = planned(N, fv.shape[1], IS, 3, options, flags, dist='barycentric')
        assert (p.form, p.threads, p.grid, p.ordered, p.both) == (_lib.SR_FORM_GENERIC, 256, N * ((IS + 15) // 16) ** 2, 0, 0)
        settings(options, flags)
        img = render(cuda, fv, ft, IS, kwg)
        assert np.abs(img - oracle.forward(fv, ft, IS, **kwg)['soft_colors']).max() <= IMG_TOL


def test_the_plan_s_device_side_choice_is_what_the_workspace_holds(settings, cuda):
    # 6 frames of 64x64 = 384 tiles (test_forward_kernel_choice_gpu.py: the bounding boxes cover about half of them)
    N, IS = 6, 64
    fv, ft, kw = batch(N, 3)
    F = fv.shape[1]

    def peek():
        return rh.peek_choice(cuda, N, F)

    settings(*FORMS[_lib.SR_FORM_ONE_WAVE][:2])
    want = render(cuda, fv, ft, IS, kw)
    # fixed tile order: sr_choose_kernel writes the kernel's id -- four waves (1) while its estimate is at most coop_max
    seen = {}
    for coop_max in (300, 40):
        options = (0, coop_max, BIG, 0, BIG)
        p = planned(N, F, IS, 3, options, 0)
        assert (p.form, p.both, p.choice_source, p.ordered) == (_lib.SR_FORM_FOUR_WAVES, 1, _lib.SR_CHOICE_BBOX_ESTIMATE, 0)
        assert p.choice_max < 0 and p.choose_threshold == coop_max and (p.grid, p.threads) == (384, 256)
        settings(options, 0)
        got = render(cuda, fv, ft, IS, kw)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        seen[coop_max] = peek()
    assert seen == {300: 1, 40: 0}, seen
    # the launch's own order: sr_order_kernel leaves its count of non-empty tiles, four waves while it is at most 3/8 of coop_max
    counts = {}
    for coop_max in (660, 120):                          # x 4/7 = 376 and 68 < 384 tiles: left to the device either way
        options = (0, coop_max, BIG, BIG, BIG)
        p = planned(N, F, IS, 3, options, 0)
        assert (p.form, p.both, p.choice_source, p.ordered) == (_lib.SR_FORM_FOUR_WAVES, 1, _lib.SR_CHOICE_NONEMPTY_TILES, 1)
        assert p.choice_max == coop_max // 8 * 3 and (p.tile_shift, p.tso, p.order_groups) == (3, 8, 1)
        settings(options, 0)
        got = render(cuda, fv, ft, IS, kw)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        counts[coop_max] = peek()
    busy = counts[660]
    print('non-empty tiles: %d of 384; bounds %d and %d' % (busy, 660 // 8 * 3, 120 // 8 * 3))
    assert counts[120] == busy and 120 // 8 * 3 < busy <= 660 // 8 * 3, counts       # so the two settings took different kernels
