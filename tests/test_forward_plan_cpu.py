"""Which forward kernel a launch takes, in which tile order and with what geometry is decided by plan_forward
(lasr_amd/csrc/sr_raster.hip), a pure function of the call's sizes, modes, flags and options; lasr_sr_plan_forward exposes it
without a launch, so the arithmetic that applies the measured thresholds runs here, without a GPU.  The rows were worked out by
hand from the expressions with the built-in defaults: eight waves up to 2200 8x8 tiles, four up to 14336, the device decides up to
49152, the pair walk from 3072 8x8 tiles (two teams up to 3072 16x16 tiles), the launch's own tile order from 5 frames, groups of
4 images.  Six and nine channels take 5/8 of the first two bounds and no device-decided range; ordered launches of three channels
take four waves up to 14336 / 7 * 4 = 8192 tiles and let the device decide up to 49152 / 16 * 7 = 21504."""
import ctypes
import os

import numpy as np
import pytest

from lasr_amd import _lib

ENV = ('LASR_SR_COOP8_MAX_TILES', 'LASR_SR_COOP_MAX_TILES', 'LASR_SR_CHOOSE_MAX_TILES', 'LASR_SR_ORDER_MAX_TILES',
       'LASR_SR_ORDER_MIN_FRAMES', 'LASR_SR_ORDER_GROUP_IMAGES', 'LASR_SR_PAIR_MIN_TILES', 'LASR_SR_PAIR_TEAMS_MAX_TILES')
pytestmark = pytest.mark.skipif(any(n in os.environ for n in ENV),
                                reason='the rows assume the built-in thresholds: a LASR_SR_* override of them is set')

HUGE = 10 ** 12
GENERIC, ONE_WAVE, RELAXED, FOUR, EIGHT, SEG_FOUR, SEG_EIGHT, PAIRS_ONE, PAIRS_TWO = range(9)
NONE, BBOX, NONEMPTY = range(3)
THREADS = {GENERIC: 256, ONE_WAVE: 64, RELAXED: 64, FOUR: 256, EIGHT: 512, SEG_FOUR: 256, SEG_EIGHT: 512, PAIRS_ONE: 256, PAIRS_TWO: 512}
TILE_AREA = {GENERIC: 256, PAIRS_ONE: 256, PAIRS_TWO: 256}                 # the others: 8x8


def plan(N, F=2420, IS=256, nch=3, flags=0, dist=2, rc=0, **options):
    o = _lib.SrOptions(*[options.get(n, -1) for n, _ in _lib.SrOptions._fields_])
    p = _lib.SrPlan()
    got = _lib.lib().lasr_sr_plan_forward(N, F, 3, nch, IS, dist, 1, 2, 1, 1, flags, ctypes.byref(o) if options else None, ctypes.byref(p))
    assert got == rc, (got, rc)
    return p


def test_the_mirror_names_the_header_s_forms():
    assert (GENERIC, ONE_WAVE, RELAXED, FOUR, EIGHT, SEG_FOUR, SEG_EIGHT, PAIRS_ONE, PAIRS_TWO) == (
        _lib.SR_FORM_GENERIC, _lib.SR_FORM_ONE_WAVE, _lib.SR_FORM_ONE_WAVE_RELAXED, _lib.SR_FORM_FOUR_WAVES, _lib.SR_FORM_EIGHT_WAVES,
        _lib.SR_FORM_SEG_FOUR, _lib.SR_FORM_SEG_EIGHT, _lib.SR_FORM_PAIRS_ONE_TEAM, _lib.SR_FORM_PAIRS_TWO_TEAMS)
    assert (NONE, BBOX, NONEMPTY) == (_lib.SR_CHOICE_NONE, _lib.SR_CHOICE_BBOX_ESTIMATE, _lib.SR_CHOICE_NONEMPTY_TILES)


def test_default_plan_of_the_bench_object_by_frame_count():
    # 2420 faces at 256x256: 1024 8x8 tiles and 256 16x16 tiles per frame
    for N in (1, 2):
        p = plan(N)
        assert (p.form, p.threads, p.grid, p.ordered, p.both) == (EIGHT, 512, 1024 * N, 0, 0)
    p = plan(3)                                                   # 3072 tiles: the pair walk, too few frames for the order
    assert (p.form, p.threads, p.grid, p.ordered) == (PAIRS_TWO, 512, 768, 0)
    p = plan(8)
    assert (p.form, p.ordered, p.tile_shift, p.tso, p.order_groups, p.grid) == (PAIRS_TWO, 1, 4, 16, 1, 2048)
    assert plan(12).form == PAIRS_TWO                              # 3072 16x16 tiles: the last launch with two teams
    p = plan(13)
    assert (p.form, p.threads, p.grid, p.ordered) == (PAIRS_ONE, 256, 3328, 1)
    p = plan(256)                                                  # 32 images per XCD, 14.9 MB of records: groups of 4 images
    assert (p.form, p.ordered, p.order_groups, p.grid) == (PAIRS_ONE, 1, 8, 65536)
    for N in (1, 2, 3, 8, 12, 13, 256):
        p = plan(N)
        assert (p.both, p.choice_source, p.choice_max) == (0, NONE, -1)


def test_segmented_and_relaxed_flags():
    assert plan(1, flags=_lib.SR_SEGMENTED).form == SEG_EIGHT
    assert plan(3, flags=_lib.SR_SEGMENTED).form == SEG_FOUR      # 3072 > 2200, at most twice 2200; the flag keeps the pair walk away
    assert plan(5, flags=_lib.SR_SEGMENTED).form == FOUR          # 5120 tiles is above twice 2200: the flag is ignored
    p = plan(64, flags=_lib.SR_RELAXED_MATH)
    assert (p.form, p.threads, p.grid, p.ordered, p.tile_shift, p.tso) == (RELAXED, 64, 65536, 1, 3, 32)
    # a launch the pair walk takes ignores the team flags' absence and honours their presence
    assert plan(3, flags=_lib.SR_PAIR_ONE_TEAM).form == PAIRS_ONE and plan(64, flags=_lib.SR_PAIR_TWO_TEAMS).form == PAIRS_TWO


def test_the_8x8_tile_kernels_without_the_pair_walk():
    off = dict(pair_min_tiles=HUGE)
    p = plan(3, **off)
    assert (p.form, p.ordered, p.both) == (FOUR, 0, 0)
    p = plan(8, **off)                                            # 8192 <= 14336 / 7 * 4 = 8192
    assert (p.form, p.ordered, p.both, p.tile_shift, p.tso) == (FOUR, 1, 0, 3, 32)
    for N in (9, 21):                                             # 21504 <= 49152 / 16 * 7 = 21504
        p = plan(N, **off)
        assert (p.form, p.both, p.choice_source, p.choice_max, p.ordered) == (FOUR, 1, NONEMPTY, 14336 // 8 * 3, 1)
        assert p.choice_max == 5376 and p.grid == 1024 * N and p.threads == 256
    p = plan(22, **off)
    assert (p.form, p.both, p.choice_source, p.choice_max) == (ONE_WAVE, 0, NONE, -1)
    # ... and in the fixed tile order: four waves up to 14336, sr_choose_kernel's estimate up to 49152
    off = dict(pair_min_tiles=HUGE, order_max_tiles=0)
    p = plan(14, **off)
    assert (p.form, p.both, p.ordered) == (FOUR, 0, 0)
    for N in (15, 48):
        p = plan(N, **off)
        assert (p.form, p.both, p.choice_source, p.ordered) == (FOUR, 1, BBOX, 0)
        assert p.choice_max < 0 and p.choose_threshold == 14336
    p = plan(49, **off)
    assert (p.form, p.both, p.choice_source) == (ONE_WAVE, 0, NONE)


def test_nine_channels_take_five_eighths_of_the_bounds_and_never_both():
    kw = dict(F=1280, nch=9, pair_min_tiles=HUGE)
    assert plan(1, **kw).form == EIGHT                            # 1024 <= 2200 / 8 * 5 = 1375
    assert plan(2, **kw).form == FOUR
    p = plan(8, **kw)                                             # 8192 <= 14336 / 8 * 5 = 8960
    assert (p.form, p.ordered) == (FOUR, 1)
    assert plan(9, **kw).form == ONE_WAVE
    for nch in (6, 9):
        for N in range(1, 70):
            p = plan(N, F=1280, nch=nch, pair_min_tiles=HUGE)
            assert p.both == 0 and p.choice_source == NONE
    p = plan(16, F=1280, nch=9)                                   # the render of a LASR step: the pair walk by default
    assert (p.form, p.threads, p.grid) == (PAIRS_ONE, 256, 4096)


def test_other_mode_combinations_take_the_generic_kernel_whatever_the_options():
    for N, IS in ((1, 256), (7, 100), (64, 64)):
        for options in ({}, dict(pair_min_tiles=0), dict(coop8_max_tiles=HUGE, coop_max_tiles=HUGE, choose_max_tiles=HUGE), dict(order_max_tiles=HUGE)):
            for flags in (0, _lib.SR_RELAXED_MATH, _lib.SR_SEGMENTED):
                p = plan(N, IS=IS, dist=0, flags=flags, **options)
                assert (p.form, p.threads, p.grid, p.ordered, p.both) == (GENERIC, 256, N * ((IS + 15) // 16) ** 2, 0, 0)


def test_launches_the_order_and_the_pair_walk_do_not_take():
    p = plan(5, IS=100)                                           # 5 x 13 x 13 = 845 tiles: no multiple of 8
    assert p.ordered == 0 and p.grid == 845
    assert plan(8, IS=100).ordered == 1                           # 1352 tiles
    for N in (1, 5, 8, 64):
        for options in ({}, dict(pair_min_tiles=0), dict(coop8_max_tiles=0, coop_max_tiles=0, choose_max_tiles=HUGE)):
            p = plan(N, F=0, **options)                           # no faces: the kernel only writes the background
            assert p.form not in (PAIRS_ONE, PAIRS_TWO) and (p.ordered, p.both, p.choice_source) == (0, 0, NONE)


def test_refusals_and_the_empty_batch_are_the_forward_s():
    # the arguments of test_abi.py::test_argument_validation_happens_before_any_launch
    h = _lib.lib()
    p = _lib.SrPlan()
    assert h.lasr_sr_plan_forward(1, 1, 3, 3, 8, 7, 1, 2, 1, 1, 0, None, ctypes.byref(p)) == -2        # mode id out of range
    assert h.lasr_sr_plan_forward(-1, 1, 3, 3, 8, 2, 1, 2, 1, 1, 0, None, ctypes.byref(p)) == -1       # negative size
    assert h.lasr_sr_plan_forward(1, 1, 3, 3, 8, 2, 1, 2, 1, 1, 0, None, None) == -1                   # nowhere to write
    assert h.lasr_sr_plan_forward(1, 1, 3, 3, 8, 2, 1, 2, 1, 1, 64, None, ctypes.byref(p)) == -1       # not a forward flag
    assert h.lasr_sr_plan_forward(1, 1, 3, 3, 8, 2, 1, 2, 1, 1, _lib.SR_RECORDS_VALID, None, ctypes.byref(p)) == -1
    assert h.lasr_sr_plan_forward(1, 1, 3, 5, 8, 2, 1, 2, 1, 1, 0, None, ctypes.byref(p)) == -2        # five channels
    assert h.lasr_sr_plan_forward(1, 1, 3, 6, 8, 1, 1, 2, 1, 1, 0, None, ctypes.byref(p)) == -2        # six: LASR's modes only
    assert h.lasr_sr_plan_forward(1, 1, 3, 3, 8, 2, 1, 2, 1, 1, _lib.SR_DEFAULT_FLAGS, None, ctypes.byref(p)) == 0
    assert (p.form, p.threads, p.grid) == (EIGHT, 512, 1)
    for N, IS in ((0, 8), (0, 0), (3, 0)):                                                             # empty batch: a zeroed plan
        p.form = p.threads = p.choice_max = 7
        assert h.lasr_sr_plan_forward(N, 1, 3, 3, IS, 2, 1, 2, 1, 1, 0, None, ctypes.byref(p)) == 0
        assert bytes(p) == bytes(ctypes.sizeof(p))


def test_properties_of_random_plans():
    rng = np.random.default_rng(10)
    pick = lambda: int(rng.choice([-1, 0, int(rng.integers(1, 100000)), HUGE]))
    seen = set()
    for _ in range(600):
        N, IS = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        F = int(rng.choice([0, 1, 63, 64, 65, 1280, 2420, 7220]))
        nch = int(rng.choice([3, 3, 6, 9]))
        dist = 2 if nch > 3 else int(rng.choice([2, 2, 2, 0, 1]))
        flags = int(rng.choice([0, 0, 1, 2, 3, 16, 32, 18]))
        options = dict(coop8_max_tiles=pick(), coop_max_tiles=pick(), choose_max_tiles=pick(), order_max_tiles=pick(), pair_min_tiles=pick())
        p = plan(N, F=F, IS=IS, nch=nch, flags=flags, dist=dist, **options)
        seen.add(p.form)
        assert p.grid * TILE_AREA.get(p.form, 64) >= N * IS * IS             # the grid covers the image ...
        side = 16 if p.form in TILE_AREA else 8
        assert p.grid == N * ((IS + side - 1) // side) ** 2                   # ... with one block per tile
        assert p.threads == THREADS[p.form]
        assert not p.both or (nch == 3 and p.form in (FOUR, SEG_FOUR) and p.choice_source in (BBOX, NONEMPTY))
        assert (p.choice_source == NONE) == (not p.both) and (p.choice_max >= 0) == (p.choice_source == NONEMPTY)
        assert (p.choice_source == NONEMPTY) <= bool(p.ordered)
        assert p.tile_shift == (4 if p.form in (PAIRS_ONE, PAIRS_TWO) else 3) and p.tso == (IS + (1 << p.tile_shift) - 1) >> p.tile_shift
        if p.ordered:
            assert N >= 5 and (N * p.tso * p.tso) % 8 == 0 and F > 0 and p.form != GENERIC
            assert p.order_groups >= 1 and (p.order_groups == 1 or (N % 8 == 0 and (N // 8) % p.order_groups == 0))
        if dist != 2:
            assert p.form == GENERIC
    assert seen == set(range(9)), seen
